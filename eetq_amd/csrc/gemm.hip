// Fused int8-dequant + fp16 MFMA GEMM for prefill (M >= 5), gfx950.
//
// Replaces the reference's CUTLASS path: ft::gemm_fp16_int (csrc/cutlass_kernels/fpA_intB_gemm.cu:21-33) ->
// GemmFpAIntB / DqMmaMultistage (csrc/cutlass_extensions/.../gemm/kernel/fpA_intB_gemm.h:296-462,
// gemm/threadblock/dq_mma_multistage.h:310-590).  Numerics contract kept from that code: int8 -> fp16 exact,
// multiplied by the per-column fp16 scale in registers *before* the matrix instruction
// (mma_tensorop_dequantizer.h:259-274), fp32 accumulation (default_fpA_intB_traits.h:110), fp16 store with
// alpha = 1, beta = 0 (epilogue_helpers.h:73-80).  Nothing else is shared with it.
//
// Structure (details in gemm_kernel.hpp):
//   * workgroup tile 128(M) x 128(N), K step 64; 4 waves = 2 K halves x 2 column halves; a wave owns 128 rows x
//     64 columns of one 32-deep K half, so each dequantised weight fragment is reused by 4 MFMAs (M-repeat) and each
//     activation fragment by 2 (N-repeat) -- the int8->fp16 VALU work and the LDS reads are the scarce resources;
//   * v_mfma_f32_32x32x16_f16 with the weights as the A operand (4 consecutive accumulators = 4 consecutive n of one
//     token: 8-byte fp16 stores, no transpose), 128 fp32 accumulators per lane; the two K halves are added once in LDS;
//   * A (fp16 activations) and B (uint8 native tiles) are staged HBM/L2 -> LDS with buffer_load_dwordx4 ... lds
//     (LDS-DMA, no VGPR round trip), 6-stage ring, one s_barrier per K step, counted vmcnt;
//   * A's LDS image is XOR-swizzled through the *source* address (key (row>>1)&7 on the 16-byte slot): ds_read_b128 of
//     32 rows at one k offset is conflict-free; B's LDS image is the lane-linear global tile, conflict-free as is;
//   * LDS -> register fragment reads, the dequant of the next K step and the DMA of stage kt+5 are hand-placed in the
//     shadow of the current step's MFMAs (sched_barrier-pinned issue order, see gemm_kernel.hpp);
//   * blockIdx -> tile mapping gives each XCD (own L2) a contiguous run of tiles ordered in groups of 4 row tiles: the
//     32 workgroups resident on an XCD cover 4 row tiles x 8 column tiles, the smallest fabric footprint per K step.
//
// Host side: launch_gemm_mfma walks the launch plan of gemm_tile_plan.hpp -- row chunks below 2 GiB, the wide or the narrow tile by
// the cost rule, whole rounds of wide tiles and the ragged last round -- through gemm_tile_launch.hpp, which applies every pointer
// and epilogue offset; this file supplies the int8 limits, the kernel tables and the K-sliced launch of a ragged round.  The plan
// is shared with gemm_int4_tiled.hip and, for the tile rule, with the grouped forms; eetq_diag_tile_plan (abi.hip) shows it.
#include <cstdio>
#include <cstdlib>

#include "gemm_tile_launch.hpp"

namespace eetq {

using namespace gemm;

bool splitk_allowed()
{
    static const bool allowed = [] {  // EETQ_AMD_SPLITK=0: no library-owned scratch anywhere (gemm_splitk.hip)
        const char* e = getenv("EETQ_AMD_SPLITK");
        return !(e && e[0] == '0');
    }();
    return allowed;
}

namespace {
// The calling stream's split-K region for `tiles` tiles of width bn in S (2 or 4) slices: its slabs and the ticket array of S.
// EETQ_ERR_UNSUPPORTED (no message): the stream has no scratch of its own right now, or not enough of it.
int tile_splitk_region(hipStream_t stream, int tiles, int bn, int S, float** slabs, unsigned** tickets)
{
    unsigned *t2 = nullptr, *t4 = nullptr;
    size_t    slab_bytes = 0, max_tiles = 0;
    const int st = splitk_region(stream, slabs, &slab_bytes, &t2, &t4, &max_tiles);
    if (st != EETQ_OK) return st;
    if ((size_t)tiles > max_tiles || (size_t)tiles * S * BM * bn * 4 > slab_bytes) return EETQ_ERR_UNSUPPORTED;
    *tickets = S == 2 ? t2 : t4;
    return EETQ_OK;
}

// S (2 or 4) K slices of the 128 x 64 tile over one column segment of the plan (operands already moved to it).
// EETQ_ERR_UNSUPPORTED (no message): the caller runs those columns unsplit.
int launch_tile_splitk_cols(const TileLaunch& t, int K, int S, hipStream_t stream)
{
    if (!splitk_allowed() || (S != 2 && S != 4) || t.ep.act != 0 || K % BK != 0 || (K / BK) / S < kMinKSteps) return EETQ_ERR_UNSUPPORTED;
    const int tiles = tile_plan::row_tiles(t.rows) * tile_plan::ceil_div(t.seg.cols, TileCfg<1>::BN);  // narrow, whatever shape the fall-back has
    float*    slabs   = nullptr;
    unsigned* tickets = nullptr;
    const int st      = tile_splitk_region(stream, tiles, TileCfg<1>::BN, S, &slabs, &tickets);
    if (st != EETQ_OK) return st;
    static LargeLdsKernel<decltype(&gemm_tile_splitk_kernel<1>)> kernel{gemm_tile_splitk_kernel<1>};
    return launch_large_lds(kernel, "gemm_tile_splitk_kernel launch", dim3(tiles * S), dim3(256), TileCfg<1>::SMEM_BYTES, stream, t.x, t.w,
                            t.scales, t.y, t.rows, t.seg.cols, K, t.ldc, t.ep, S, slabs, tickets);
}
}  // namespace

int launch_gemm_mfma(const f16* x, const uint8_t* w, const f16* scales, Epilogue ep, f16* y, int M, int N, int K,
                     hipStream_t stream)
{
    // kActGlu8: the weight's columns are gate / up groups of 8 + 8 and y is [M][N / 2] (gemm_kernel.hpp, GLU); no residual
    const bool glu = ep.act == kActGlu8;
    if (glu && (!tile_plan::deep_enough(8, K) || N % 16 != 0 || ep.residual)) return EETQ_ERR_UNSUPPORTED;  // quiet: the caller runs two launches
    if (!tile_plan::deep_enough(8, K))
        // K < 320: a few KiB of weights per column tile; run the stream kernel over 64-row chunks instead of carrying a
        // second tiled kernel for it (the weights are re-read from L2, the activations are read once)
        return tile_plan::for_each_row_chunk(M, kStreamMaxM, [&](int m, int rows) {
            Epilogue e = ep;
            if (e.residual) e.residual += (size_t)m * N;
            return launch_streamk(x + (size_t)m * K, w, scales, e, y + (size_t)m * N, rows, N, K, stream);
        });
    // the LDS-DMA path addresses its operands with 32-bit buffer offsets; the activations go in row chunks below 2 GiB
    EETQ_REQUIRE(tile_plan::weight_fits(8, N, K), "weight larger than 2 GiB is not supported by the buffer-addressed DMA path");
    EETQ_REQUIRE(tile_plan::max_rows(K) >= BM, "K too large for the buffer-addressed DMA path");
    // the plan's launches (gemm_tile_plan.hpp); K slices of the ragged round under the identity epilogue only
    return for_each_tile_launch(8, x, w, scales, ep, y, M, N, K, device_cu_count(), 0, ep.act == 0, [&](const TileLaunch& t) {
        const int st = t.seg.k_slices > 1 ? launch_tile_splitk_cols(t, K, t.seg.k_slices, stream) : EETQ_ERR_UNSUPPORTED;
        if (st != EETQ_ERR_UNSUPPORTED) return st;
        // [narrow][identity / activation epilogue / GLU write-out], each its own instantiation (gemm_kernel.hpp).  > 64 KiB of
        // dynamic LDS: the kernel about to be launched is opted in, once per device (common.hpp)
        static LargeLdsKernel<decltype(&gemm_tile_kernel<0, 2>)> kernels[2][3] = {
            {{gemm_tile_kernel<0, 2>}, {gemm_tile_kernel<0, 2, true>}, {gemm_tile_kernel<0, 2, false, 2, true>}},
            {{gemm_tile_kernel<0, 1>}, {gemm_tile_kernel<0, 1, true>}, {gemm_tile_kernel<0, 1, false, 2, true>}}};
        return launch_large_lds(kernels[t.seg.narrow][glu ? 2 : t.ep.act != 0], "gemm_tile_kernel launch", dim3(tile_plan::grid_of(t.rows, t.seg)),
                                dim3(256), tile_plan::lds_bytes(t.seg.narrow, 8), stream, t.x, t.w, t.scales, t.y, t.rows, t.seg.cols, K, t.ldc,
                                t.ep);
    });
}

// ---- K slices of the 128 x 64 tile ------------------------------------------------------------------------------------
// The tiled kernel runs ONE workgroup per tile: M <= 128 at N = 4096 is 64 tiles on 256 CUs (20.6 us at M = 128), M = 256 is
// 128.  With S workgroups per tile, each on a contiguous S-th of the K steps, the chip fills and the per-workgroup loop
// shortens S-fold; the price is the hand-over of S partial tiles (32 KiB each) to the workgroup that finishes last.
int tile_splitk_slices(int M, int N, int K)
{
    const int ncu   = device_cu_count();
    const int tiles = ((M + BM - 1) / BM) * ((N + TileCfg<1>::BN - 1) / TileCfg<1>::BN);
    const int KT    = K / BK;
    // Every workgroup must get a CU of its own (a second round costs more than the slices save: M = 256 at 5120^2, 160 tiles,
    // 35.8 us with two slices vs 27.6 unsplit), and the hand-over (~3.5 us: publish, ticket, read-back of S slabs) must be
    // small against the loop it shortens -- measured (tools/experiments/tilesplit_check.py, graph-replayed chains, us,
    // split vs best other path):
    //   four slices of 43 steps:  M = 128 at 11008 x 4096 23.9 vs 27.1, M = 100 23.3 vs 25.6
    //   two slices of >= 40:      M = 128 at 5120^2 20.1 vs 22.6, 13824 x 5120 40.9 vs 46.8, M = 256 at 11008 x 4096 37.1 vs 54.4
    //   four slices of 16:        M = 97..128 at 4096^2 13.5 vs 15.5 on one box, 15.3-15.8 vs 15.0-15.5 on two others: not taken
    //   two slices of 32:         M = 160 at 4096^2 17.7 vs 16.7, M = 256 19.8 vs 20.9: not taken
    if (tiles * 4 <= ncu && KT / 4 >= 24) return 4;
    if (tiles * 2 <= ncu && KT / 2 >= 40) return 2;
    return 1;
}

// the same question for the 128 x 128 tile (two slices at most: its partial tile is 64 KiB): M = 257..512 on N <= 4096, where
// whole wide tiles cover half the chip and the narrow tiles that fill it cost 0.70 of a wide pass each.  The 64 KiB hand-over
// is dearer (~6 us), so only very deep K pays: M = 512 at 11008 x 4096 (86 steps per slice) 51.7 vs 58.3 us; at 4096^2 (32)
// 27.8 vs 23.2, 8192 x 4096 (64) 40.6 vs 40.0: not taken.
int wide_tile_splitk_slices(int M, int N, int K)
{
    const int ncu   = device_cu_count();
    const int tiles = ((M + BM - 1) / BM) * ((N + TileCfg<2>::BN - 1) / TileCfg<2>::BN);
    const int KT    = K / BK;
    return (tiles * 2 <= ncu && tiles * 4 > ncu && KT / 2 >= 80) ? 2 : 1;
}

int launch_gemm_tile_splitk(const f16* x, const uint8_t* w, const f16* scales, Epilogue ep, f16* y, int M, int N, int K,
                            hipStream_t stream, int force_s, int* used_s, bool env_plan)
{
    if (used_s) *used_s = 1;
    const bool allowed = splitk_allowed();
    int S = !allowed ? 1 : (force_s ? force_s : tile_splitk_slices(M, N, K));
    bool wide = false;
    if (allowed && !force_s && S == 1 && wide_tile_splitk_slices(M, N, K) == 2) {
        S    = 2;
        wide = true;
    }
    // EETQ_AMD_TILESPLIT_PLAN="S" overrides the slice count of the 128 x 64 tile on the explicitly FORCED path only
    // (EETQ_PATH_TILESPLIT: tuning and tests, read per call); AUTO launches never read it
    if (const char* e = (env_plan && allowed) ? getenv("EETQ_AMD_TILESPLIT_PLAN") : nullptr) {
        int a = 0;
        if (sscanf(e, "%d", &a) == 1) {
            S    = a;
            wide = false;
        }
    }
    const bool fits = (size_t)M * K * 2 < (1ull << 31) && (size_t)N * K < (1ull << 31);
    if ((S != 2 && S != 4) || ep.act != 0 || !fits || K % BK != 0 || (K / BK) / S < kMinKSteps)
        return launch_gemm_mfma(x, w, scales, ep, y, M, N, K, stream);
    const int BN    = wide ? TileCfg<2>::BN : TileCfg<1>::BN;
    const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    float*    slabs   = nullptr;
    unsigned* tickets = nullptr;
    int       st      = tile_splitk_region(stream, tiles, BN, S, &slabs, &tickets);
    if (st == EETQ_ERR_UNSUPPORTED) return launch_gemm_mfma(x, w, scales, ep, y, M, N, K, stream);  // no scratch of its own for this stream: unsplit
    if (st != EETQ_OK) return st;
    static LargeLdsKernel<decltype(&gemm_tile_splitk_kernel<1>)> kernels[2] = {{gemm_tile_splitk_kernel<1>}, {gemm_tile_splitk_kernel<2>}};
    st = launch_large_lds(kernels[wide], "gemm_tile_splitk_kernel launch", dim3(tiles * S), dim3(256),
                          wide ? TileCfg<2>::SMEM_BYTES : TileCfg<1>::SMEM_BYTES, stream, x, w, scales, y, M, N, K, N, ep, S, slabs, tickets);
    if (st == EETQ_OK && used_s) *used_s = S;
    return st;
}

}  // namespace eetq
