// Kernel template of the grouped decode GEMM over a routed expert stack, and what its two translation units
// share: moe.hip instantiates BITS = 8 ([E][K][N] int8), moe_int4.hip BITS = 4 ([E][K][N / 2] packed int4).
#pragma once
#include "common.hpp"
#include "gemv_kernel.hpp"

namespace eetq {

constexpr int kMoeMaxExperts = 1024;  // eetq_moe_route's limit

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// the argument checks eetq_w8a16_moe_gemm, eetq_w8a16_moe_gemm_tiled and eetq_w4a16_moe_gemm share (`fn` names the entry in the
// messages, `bits` picks the layout's k depth); defined in moe.hip
int moe_gemm_check(const char* fn, int bits, const void* x, const int8_t* w_packed, const void* scales, const int* offsets,
                   const int* sorted_slot, const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8);

struct MoeGemmArgs {
    const f16*     x;
    const uint8_t* w;
    const f16*     s;
    const int *    offsets, *sorted_slot, *active;
    f16*           y;
    int            topk, A, N, K;
    bool           gather, glu8;
    hipStream_t    stream;
};

// the grouped entries' (checked) arguments as the launcher takes them: A = min(E, T k) active slots
inline MoeGemmArgs moe_gemm_args(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                                 const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream)
{
    const int S = T * k;
    return {static_cast<const f16*>(x), reinterpret_cast<const uint8_t*>(w_packed), static_cast<const f16*>(scales), offsets,
            sorted_slot, active, static_cast<f16*>(y), k, S < E ? S : E, N, K, gather != 0, glu8 != 0, static_cast<hipStream_t>(stream)};
}

// Grouped GEMM over the expert stack: the small-batch stream kernel's body (streamk_kernel.hpp, one row tile, activations straight
// from global memory: XM = 0) with a row map.  blockIdx.y = active slot a (exit on -1), blockIdx.x = 16-column tile row.
// Rows of expert e: sorted positions offsets[e] .. offsets[e + 1] - 1, taken 16 at a time (one MFMA row tile; T <= 16 needs one).
// Row p reads x[sorted_slot[p] / k] (GATHER) or x[p], and writes y[p].  The expert's weight tile row (K / kTileK tiles of 1 KiB) is
// streamed once per 16 rows.  A stage is one 16-byte weight vector (kLaneK k of the lane's column) + kXQ activation vectors (the
// same k of the lane's row): int8 two v_mfma_f32_16x16x32_f16 on the dequantised halves, int4 four, dword d of the weight vector
// against activation vector d.
// GLU8: columns in glu8 order (8 gate + the matching 8 up per 16-column tile), y[p][8 tile + c] = silu_mul(gate, up) -- the
// streamk kernel's glu8 epilogue, i.e. the projection followed by eetq_silu_mul_glu8_f16, bit for bit.
// The instantiations have external linkage (a header template): each BITS value is instantiated in one translation unit only,
// so that no two objects built with different flags can define the same kernel.
template <int BITS, int WAVES, int D, bool GATHER, bool GLU8>
__global__ __launch_bounds__(WAVES * 64) void moe_gemm_kernel(const f16* __restrict__ x, const uint8_t* __restrict__ w_all,
                                                               const f16* __restrict__ scales_all, const int* __restrict__ offsets,
                                                               const int* __restrict__ sorted_slot, const int* __restrict__ active,
                                                               f16* __restrict__ y, int topk, int N, int K)
{
    using CD = gemv::Codec<BITS>;
    const int e = active[blockIdx.y];
    if (e < 0) return;
    const int p0 = offsets[e], rows = offsets[e + 1] - p0;

    __shared__ float red[WAVES * 256];
    const int tid  = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int KT    = K / CD::kTileK;
    const int ntile = blockIdx.x;

    const uint8_t* w      = w_all + (size_t)e * K * (BITS == 8 ? N : N >> 1);
    const f16*     scales = scales_all + (size_t)e * N;
    const u32      sraw   = reinterpret_cast<const uint16_t*>(scales)[ntile * 16 + c];
    const u32x4*   wp     = reinterpret_cast<const u32x4*>(w + (size_t)ntile * KT * kTileBytes) + lane;  // + 64 per k tile

    for (int r0 = 0; r0 < rows; r0 += 16) {
        // lane (g, c) feeds row r0 + c (clamped: rows beyond the expert's compute garbage that is never stored)
        const int rc = r0 + c < rows ? r0 + c : rows - 1;
        const int xr = GATHER ? sorted_slot[p0 + rc] / topk : p0 + rc;
        const u32x4* xrow = reinterpret_cast<const u32x4*>(x + (size_t)xr * K + CD::kLaneK * g);  // + kTileK / 8 u32x4 per k tile

        struct Stage {
            u32x4 wq, xa[CD::kXQ];
        };
        // the two loads keep their own form: one loop over kXQ costs the int8 1 x 1 instantiations an instruction or two
        auto load_stage = [&](int kt, Stage& s) {
            s.wq = gemv::load_w<true>(wp + (size_t)kt * 64);
            if constexpr (BITS == 8) {
                s.xa[0] = xrow[(size_t)kt * 8];
                s.xa[1] = xrow[(size_t)kt * 8 + 1];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) s.xa[q] = xrow[(size_t)kt * 16 + q];
            }
        };
        f32x4       acc    = {0.f, 0.f, 0.f, 0.f};
        const f16x2 scale2 = as_f16x2(sraw | (sraw << 16));
        auto consume = [&](const Stage& s) {
            if constexpr (BITS == 8) {
                f16x2 wq[8];
                dequant_16(s.wq, scale2, wq);
                const f16x8 b0 = {wq[0].x, wq[0].y, wq[1].x, wq[1].y, wq[2].x, wq[2].y, wq[3].x, wq[3].y};
                const f16x8 b1 = {wq[4].x, wq[4].y, wq[5].x, wq[5].y, wq[6].x, wq[6].y, wq[7].x, wq[7].y};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, s.xa[0]), b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, s.xa[1]), b1, acc, 0, 0, 0);
            } else {
                const u32 wd[4] = {s.wq.x, s.wq.y, s.wq.z, s.wq.w};  // dword d = k values 8d .. 8d + 7 of the lane
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    f16x2 wq[4];
                    gemv::dequant_dword_i4(wd[d], scale2, wq);
                    const f16x8 b = {wq[0].x, wq[0].y, wq[1].x, wq[1].y, wq[2].x, wq[2].y, wq[3].x, wq[3].y};
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, s.xa[d]), b, acc, 0, 0, 0);
                }
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

// grid = 16-column tile rows x active slots; every wave must own >= D k tiles (the caller's plan rule)
template <int BITS, int WAVES, int D>
int launch_moe_gemm_inst(const MoeGemmArgs& a)
{
    const dim3 grid(a.N / kTileN, a.A), block(WAVES * 64);
    auto go = [&](auto kern) {
        launch_kernel(kern, grid, block, 0, a.stream, a.x, a.w, a.s, a.offsets, a.sorted_slot, a.active, a.y, a.topk, a.N, a.K);
    };
    if (a.gather)
        a.glu8 ? go(moe_gemm_kernel<BITS, WAVES, D, true, true>) : go(moe_gemm_kernel<BITS, WAVES, D, true, false>);
    else
        a.glu8 ? go(moe_gemm_kernel<BITS, WAVES, D, false, true>) : go(moe_gemm_kernel<BITS, WAVES, D, false, false>);
    return check_hip(hipGetLastError(), "moe_gemm_kernel launch");
}

}  // namespace eetq
