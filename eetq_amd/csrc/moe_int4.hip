// Grouped W4A16 GEMM over an [E][K][N / 2] int4 expert stack for decode: moe.hip's moe_gemm_kernel -- the routing
// tables, the grid rule, the row loop, the gather / contiguous row map and the plain / glu8 write-out -- on int4 tiles, i.e. the
// small-batch stream kernel's one-row-tile register body for BITS = 4 (streamk_kernel.hpp: XM = 0) with a row map.  A file of its
// own so that the int8 kernels' machine code in moe.o / moe_gemm_tiled.o does not depend on it.
#include <cstdio>
#include <string>

#include "common.hpp"
#include "gemv_kernel.hpp"

namespace eetq {

namespace {

constexpr int kMoeMaxExperts = 1024;  // eetq_moe_route's limit
constexpr int kTileK4        = gemv::Codec<4>::kTileK;  // 128: k per 1 KiB int4 tile (16 columns x 128 k, 32 k per lane)

// blockIdx.y = active slot a (exit on -1), blockIdx.x = 16-column tile row.  Rows of expert e: sorted positions offsets[e] ..
// offsets[e + 1] - 1, taken 16 at a time (one MFMA row tile); the expert's weight tile row (K / 128 tiles of 1 KiB) is streamed
// once per 16 rows.  Row p reads x[sorted_slot[p] / k] (GATHER) or x[p], and writes y[p].  A stage is one 16-byte weight vector
// (32 k of the lane's column) + four activation vectors (the same 32 k of the lane's row) and four v_mfma_f32_16x16x32_f16:
// dword d of the weight vector against activation vector d.  GLU8: columns in glu8 order, y[p][8 tile + c] = silu_mul(gate, up)
// -- the projection followed by eetq_silu_mul_glu8_f16, bit for bit.
template <int WAVES, int D, bool GATHER, bool GLU8>
__global__ __launch_bounds__(WAVES * 64) void moe_gemm_i4_kernel(const f16* __restrict__ x, const uint8_t* __restrict__ w_all,
                                                                  const f16* __restrict__ scales_all, const int* __restrict__ offsets,
                                                                  const int* __restrict__ sorted_slot, const int* __restrict__ active,
                                                                  f16* __restrict__ y, int topk, int N, int K)
{
    const int e = active[blockIdx.y];
    if (e < 0) return;
    const int p0 = offsets[e], rows = offsets[e + 1] - p0;

    __shared__ float red[WAVES * 256];
    const int tid  = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int KT    = K / kTileK4;
    const int ntile = blockIdx.x;

    const uint8_t* w      = w_all + (size_t)e * K * (N >> 1);
    const f16*     scales = scales_all + (size_t)e * N;
    const u32      sraw   = reinterpret_cast<const uint16_t*>(scales)[ntile * 16 + c];
    const u32x4*   wp     = reinterpret_cast<const u32x4*>(w + (size_t)ntile * KT * kTileBytes) + lane;  // + 64 per k tile

    for (int r0 = 0; r0 < rows; r0 += 16) {
        // lane (g, c) feeds row r0 + c (clamped: rows beyond the expert's compute garbage that is never stored)
        const int rc = r0 + c < rows ? r0 + c : rows - 1;
        const int xr = GATHER ? sorted_slot[p0 + rc] / topk : p0 + rc;
        const u32x4* xrow = reinterpret_cast<const u32x4*>(x + (size_t)xr * K + 32 * g);  // + 16 u32x4 per k tile

        struct Stage {
            u32x4 wq, xa[4];
        };
        auto load_stage = [&](int kt, Stage& s) {
            s.wq = gemv::load_w<true>(wp + (size_t)kt * 64);
#pragma unroll
            for (int q = 0; q < 4; ++q) s.xa[q] = xrow[(size_t)kt * 16 + q];
        };
        f32x4       acc    = {0.f, 0.f, 0.f, 0.f};
        const f16x2 scale2 = as_f16x2(sraw | (sraw << 16));
        auto consume = [&](const Stage& s) {
            const u32 wd[4] = {s.wq.x, s.wq.y, s.wq.z, s.wq.w};  // dword d = k values 8d .. 8d + 7 of the lane
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                f16x2 wq[4];
                gemv::dequant_dword_i4(wd[d], scale2, wq);
                const f16x8 b = {wq[0].x, wq[0].y, wq[1].x, wq[1].y, wq[2].x, wq[2].y, wq[3].x, wq[3].y};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, s.xa[d]), b, acc, 0, 0, 0);
            }
        };

        // software-pipelined K loop over this wave's tiles (k tiles wave, wave + WAVES, ...; >= D of them by launch contract)
        const int n = (KT - wave + WAVES - 1) / WAVES;
        Stage     st[D];
#pragma unroll
        for (int d = 0; d < D; ++d) load_stage(wave + d * WAVES, st[d]);
        int i = 0;
        for (; i + 2 * D <= n; i += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                consume(st[d]);
                load_stage(wave + (i + d + D) * WAVES, st[d]);
            }
        }
        const int r = n - (i + D);
        Stage     tail[D > 1 ? D - 1 : 1];
#pragma unroll
        for (int d = 0; d < D - 1; ++d) {
            const int t = i + D + d;
            load_stage(wave + (t < n ? t : n - 1) * WAVES, tail[d]);
        }
#pragma unroll
        for (int d = 0; d < D; ++d) consume(st[d]);
#pragma unroll
        for (int d = 0; d < D - 1; ++d)
            if (d < r) consume(tail[d]);

        // cross-wave reduction: acc[j] = partial y[row 4g + j][column c]
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wave * 256 + (4 * g + j) * 16 + c] = acc[j];
        __syncthreads();
        for (int o = tid; o < 256; o += WAVES * 64) {
            const int cc = o & 15, rr = o >> 4;
            if (r0 + rr < rows) {
                const size_t p = (size_t)p0 + r0 + rr;
                if constexpr (GLU8) {
                    if (cc < 8) {
                        float sg = 0.f, su = 0.f;
#pragma unroll
                        for (int wv = 0; wv < WAVES; ++wv) {
                            sg += red[wv * 256 + o];
                            su += red[wv * 256 + o + 8];
                        }
                        y[p * (N >> 1) + ntile * 8 + cc] = silu_mul_f16((f16)sg, (f16)su);
                    }
                } else {
                    float s = 0.f;
#pragma unroll
                    for (int wv = 0; wv < WAVES; ++wv) s += red[wv * 256 + o];
                    y[p * N + ntile * 16 + cc] = (f16)s;
                }
            }
        }
        __syncthreads();  // red is rewritten by the next 16 rows
    }
}

struct MoeI4Args {
    const f16*     x;
    const uint8_t* w;
    const f16*     s;
    const int *    offsets, *sorted_slot, *active;
    f16*           y;
    int            topk, A, N, K;
    bool           gather, glu8;
    hipStream_t    stream;
};

template <int WAVES, int D>
int launch_moe_gemm_i4_inst(const MoeI4Args& a)
{
    const dim3 grid(a.N / kTileN, a.A), block(WAVES * 64);
#define EETQ_MOE_I4_LAUNCH(G, A8)                                                                                                     \
    launch_kernel(moe_gemm_i4_kernel<WAVES, D, G, A8>, grid, block, 0, a.stream, a.x, a.w, a.s, a.offsets, a.sorted_slot, a.active, \
                  a.y, a.topk, a.N, a.K)
    if (a.gather) {
        if (a.glu8) EETQ_MOE_I4_LAUNCH(true, true);
        else EETQ_MOE_I4_LAUNCH(true, false);
    } else {
        if (a.glu8) EETQ_MOE_I4_LAUNCH(false, true);
        else EETQ_MOE_I4_LAUNCH(false, false);
    }
#undef EETQ_MOE_I4_LAUNCH
    return check_hip(hipGetLastError(), "moe_gemm_i4_kernel launch");
}

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace

}  // namespace eetq

using namespace eetq;

extern "C" {

int eetq_w4a16_moe_gemm(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                        const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream)
{
    const std::string f("eetq_w4a16_moe_gemm");
    EETQ_REQUIRE(x && w_packed && scales && offsets && active && y && (sorted_slot || !gather), f + ": null pointer");
    EETQ_REQUIRE(E >= 1 && E <= kMoeMaxExperts, f + ": E must be in [1, 1024]");
    EETQ_REQUIRE(k >= 1 && k <= E, f + ": k must be in [1, E]");
    EETQ_REQUIRE(T >= 1 && (long long)T * k <= (1ll << 30), f + ": T must be >= 1 and T * k <= 2^30");
    EETQ_REQUIRE(N >= kTileN && N % kTileN == 0 && K >= kTileK4 && K % kTileK4 == 0,
                 f + ": the gfx950 int4 layout needs K % 128 == 0 and N % 16 == 0");
    EETQ_REQUIRE((gather == 0 || gather == 1) && (glu8 == 0 || glu8 == 1), f + ": gather and glu8 are 0 or 1");
    EETQ_REQUIRE((long long)T * k * K < (1ll << 40) && (long long)E * K * N < (1ll << 40), f + ": activation or weight stack too large");
    EETQ_REQUIRE(aligned16(x) && aligned16(w_packed) && aligned16(y), "x, weight and y must be 16-byte aligned");
    const int S  = T * k;
    const int KT = K / kTileK4;
    const MoeI4Args a{static_cast<const f16*>(x), reinterpret_cast<const uint8_t*>(w_packed), static_cast<const f16*>(scales),
                      offsets, sorted_slot, active, static_cast<f16*>(y), k, S < E ? S : E, N, K, gather != 0, glu8 != 0,
                      static_cast<hipStream_t>(stream)};
    // Waves per workgroup x stages in flight per wave, by k tiles (every wave must own >= D of them; an int4 tile is 128 deep).
    // Measured (tools/moe_bench.py --plan-sweep, profiles/r10_moe_int4_plans.jsonl; one MI355X, us per launch, median of 20,
    // uniform routing; "-": fewer than waves x depth k tiles):
    //   projection (k tiles)          T     8x2     8x1     4x2     4x1     6x1     3x2
    //   mixtral gate|up (32)          1     38.2    34.0    33.2    31.9    37.9    33.9
    //                                 4     74.8    64.3    64.8    59.6    71.4    62.0
    //                                 16    139.7   130.4   126.4   123.0   142.8   122.3
    //   mixtral down (112)            1     19.7    19.4    20.3    21.9    21.6    23.4
    //                                 4     34.6    33.5    36.0    33.6    34.8    37.8
    //                                 16    60.9    65.8    65.7    73.2    68.9    69.5
    //   qwen3-30b gate|up (16)        1     11.4    9.2     10.8    7.9     8.1     8.4
    //                                 4     20.2    22.8    21.2    16.6    20.1    20.6
    //                                 16    49.8    47.0    42.8    35.4    45.8    38.2
    //   qwen3-30b down (6)            1     -       -       -       7.5     9.1     9.6
    //                                 4     -       -       -       12.0    14.0    11.8
    //                                 16    -       -       -       23.1    30.2    22.8
    // Up to 32 k tiles four waves with one stage each win or tie everywhere (3 x 2 is 0.2-0.7 us ahead at three points, inside
    // the min - max spread of both); the int8 kernel's 8 x 2 wins only on the deep projection (112 tiles, from T = 16 on; a tie
    // below).  Nothing between 32 and 112 tiles was measured: the rule switches at 64.  Qwen3's down projection (6 tiles) runs on
    // four waves (two of them own two tiles), not on one.  Why the narrow single-stage form wins is not measured (no counter
    // run); the hypothesis is occupancy: at 70 VGPRs six workgroups' waves share a SIMD and hide the latency a second stage
    // would, and a narrow workgroup leaves more column tiles resident per CU.
    // 8 x 1, 4 x 2, 6 x 1 and 3 x 2 existed for that sweep only and were deleted after it (their rows stay in the profile).
    // EETQ_AMD_MOE_I4_PLAN=<waves>x<depth> (behind EETQ_AMD_TUNING=1) forces one of the four instantiations that are left, for
    // A/B runs of the switch point (tools/moe_bench.py --plan-sweep); a plan the shape cannot feed is ignored.
    static const int forced = [] {
        const char* e = tuning_env("EETQ_AMD_MOE_I4_PLAN");
        int         wv = 0, d = 0;
        return e && sscanf(e, "%dx%d", &wv, &d) == 2 ? wv * 16 + d : 0;
    }();
    if (forced && KT >= (forced >> 4) * (forced & 15)) {
        switch (forced) {
            case 8 * 16 + 2: return launch_moe_gemm_i4_inst<8, 2>(a);
            case 4 * 16 + 1: return launch_moe_gemm_i4_inst<4, 1>(a);
            case 2 * 16 + 1: return launch_moe_gemm_i4_inst<2, 1>(a);
            case 1 * 16 + 1: return launch_moe_gemm_i4_inst<1, 1>(a);
            default: break;
        }
    }
    if (KT >= 64) return launch_moe_gemm_i4_inst<8, 2>(a);
    if (KT >= 4) return launch_moe_gemm_i4_inst<4, 1>(a);
    if (KT >= 2) return launch_moe_gemm_i4_inst<2, 1>(a);
    return launch_moe_gemm_i4_inst<1, 1>(a);
}

int eetq_w8a16_moe_gemm_tiled_supported(int T, int k, int E, int N, int K, int gather)
{
    if (T < 1 || k < 1 || E < 1 || N < 1 || K < 1) return 0;
    return moe_gemm_tiled_supports(T, k, E, N, K, gather != 0) ? 1 : 0;
}

}  // extern "C"
