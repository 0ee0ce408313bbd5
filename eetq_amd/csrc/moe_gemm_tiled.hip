// Grouped form of the LDS-tiled MFMA dequant-GEMM over an [E][K][N] int8 expert stack: the prompt path of the
// routed-experts layer.  The kernel is gemm_tile_body (gemm_kernel.hpp) with its GROUPED row map -- the K loop, the ring, the gap
// placement and the epilogues are the ungrouped tile's, so an expert's rows come out as eetq_w8a16_gemm_ex(EETQ_PATH_MFMA) makes
// them from the gathered rows, bit for bit at the same tile shape.
//
//   * grid = R row-tile slots x column tiles, R = floor(S / 128) + min(E, S), S = T k: sum_e ceil(c_e / 128) <= R for any counts
//     (every expert with rows has at most one ragged tile, and the full tiles cannot exceed floor(S / 128)), so the grid depends
//     on the shapes only and the launch can be captured;
//   * slot r is the r-th row tile in the order of the active list; a workgroup finds (expert, tile) from `offsets` / `active`
//     with a wave scan and a ballot (no LDS, no barrier) and leaves before its first DMA request when the slot is surplus;
//   * tile order: the ungrouped kernel's (XCD-contiguous runs, chunks of four row-tile slots, column tiles inside a chunk): the
//     workgroups resident on an XCD cover 4 consecutive slots x 8 column tiles -- one expert's weight tiles shared by its row
//     tiles wherever an expert has several (>= 512 rows), four experts' worth of distinct tiles otherwise, which is what any
//     order must fetch there;
//   * gather = 1: row p reads x[sorted_slot[p] / k] of x [T][K]; gather = 0: x[p] of x [S][K].  Rows past the expert's count
//     read its last row and are never stored; rows at or past offsets[E] and rows of inactive experts are never written.
//   * host side: the tile rule is the dense launchers' (gemm_tile_plan.hpp) on estimated row tiles, and the launch itself -- group
//     map, narrow / wide, ldc, grid, LDS bytes -- is launch_grouped_tiles (gemm_tile_launch.hpp), shared with moe_int4_tiled.hip;
//     this file supplies the limits, the kernel table and the EETQ_AMD_MOE_TILE_J tuning hook as the forced J.
#include "gemm_tile_launch.hpp"

namespace eetq {

using namespace gemm;

namespace {

template <int J, bool GLU>
__global__ __launch_bounds__(256, 1) void moe_gemm_tile_kernel(const f16* __restrict__ x, const uint8_t* __restrict__ w,
                                                               const f16* __restrict__ scales, f16* __restrict__ y, int N, int K,
                                                               int ldc, GroupMap map)
{
    gemm_tile_body<0, J, false, 2, false, GLU, true>(x, w, scales, y, 0, N, K, ldc, Epilogue{}, 1, nullptr, nullptr, map);
}

}  // namespace

// Which tile shape: the dense launchers' cost rule (tile_plan::narrow_cheaper) on the row tiles estimated from the shapes, since
// the counts live on the device (tile_plan::grouped_row_tiles).
bool moe_tiled_narrow(int S, int E, int N) { return tile_plan::narrow_cheaper(tile_plan::grouped_row_tiles(S, E), N, device_cu_count()); }

bool moe_gemm_tiled_supports(int T, int k, int E, int N, int K, bool gather)
{
    const long long S = (long long)T * k;
    const long long x_bytes = (gather ? (long long)T : S) * K * 2;
    const long long R = S / BM + (S < E ? S : E);
    return K % BK == 0 && K / BK >= kMinKSteps && N % kTileN == 0 && (long long)N * K < (1ll << 31) &&
           x_bytes + 4096 < (1ll << 31) && R * ((N + TileCfg<1>::BN - 1) / TileCfg<1>::BN) < (1ll << 31);
}

int launch_moe_gemm_tiled(const f16* x, const uint8_t* w, const f16* scales, const int* offsets, const int* sorted_slot,
                          const int* active, f16* y, int T, int k, int E, int N, int K, bool gather, bool glu8, hipStream_t stream)
{
    if (!moe_gemm_tiled_supports(T, k, E, N, K, gather)) return EETQ_ERR_UNSUPPORTED;  // quiet: the caller runs moe_gemm_kernel
    static const int force_j = [] {  // EETQ_AMD_MOE_TILE_J = 1 / 2 (behind EETQ_AMD_TUNING): A/B runs of the two tile shapes
        const char* e = tuning_env("EETQ_AMD_MOE_TILE_J");
        return e ? atoi(e) : 0;
    }();
    // [narrow][GLU]
    static LargeLdsKernel<decltype(&moe_gemm_tile_kernel<2, false>)> kernels[2][2] = {
        {{moe_gemm_tile_kernel<2, false>}, {moe_gemm_tile_kernel<2, true>}}, {{moe_gemm_tile_kernel<1, false>}, {moe_gemm_tile_kernel<1, true>}}};
    return launch_grouped_tiles<8>(kernels, "moe_gemm_tile_kernel launch", x, w, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather, glu8,
                                   force_j, stream);
}

}  // namespace eetq
