// Routed mixture-of-experts kernels: device-side routing tables, the grouped W8A16 GEMM over an [E][K][N] int8
// expert stack that reads them (the BITS = 8 instantiations of moe_gemm_kernel.hpp), and the weighted combine; and the backward's
// combine and gated-activation steps (whose grouped input-gradient GEMM lives in gemm_t.hip and, for int4 stacks,
// in moe_gemm_t_int4.hip).  No launch needs a
// host sync, so a decode step's MoE layer (route -> gate|up GEMM with the gated activation -> down GEMM -> combine) can be
// captured in a graph; the grid of every launch depends on T, k, E, N and K only, never on the routing.
#include "moe_gemm_kernel.hpp"
#include "moe_route_tables.hpp"

namespace eetq {

namespace {

constexpr int kRouteThreads = 1024;  // 16 waves; wave w owns the w-th contiguous segment of the T*k slots
constexpr int kRouteWaves   = kRouteThreads / 64;

// One workgroup.  Dynamic LDS: kRouteWaves * E ints (per-wave, per-expert counters) + kRouteWaves ints (scan).  The two passes
// are route_tables() (moe_route_tables.hpp), which the fused router kernel (moe_router.hip) runs on its own indices as well.
__global__ __launch_bounds__(kRouteThreads) void moe_route_kernel(const int64_t* __restrict__ idx, int S, int E, int A,
                                                                   int* __restrict__ counts, int* __restrict__ offsets,
                                                                   int* __restrict__ sorted_slot, int* __restrict__ position,
                                                                   int* __restrict__ active)
{
    extern __shared__ int lds[];
    route_tables<kRouteThreads>([idx](int s) { return idx[s]; }, S, E, A, lds, counts, offsets, sorted_slot, position, active);
}

// out[t][h] = fp16( sum_{j < k, in order} fp32(y[position[t k + j]][h]) * fp32(w[t][j]) ), slots with position -1 skipped.
// grid (ceil(H / 2048), T), 256 threads x 8 columns (16-byte loads; H % 8 == 0).
template <typename WT>
__global__ __launch_bounds__(256) void moe_combine_kernel(const f16* __restrict__ y, const int* __restrict__ position,
                                                          const WT* __restrict__ wts, f16* __restrict__ out, int k, int H)
{
    const int t = blockIdx.y, h = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (h >= H) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
        const int p = position[(size_t)t * k + j];
        if (p < 0) continue;
        const float wj = (float)wts[(size_t)t * k + j];
        const u32x4 v  = *reinterpret_cast<const u32x4*>(y + (size_t)p * H + h);
        const u32   d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f16x2 pr = as_f16x2(d[q]);
            acc[2 * q] += (float)pr.x * wj;
            acc[2 * q + 1] += (float)pr.y * wj;
        }
    }
    u32x4 o;
    o.x = as_u32(f16x2{(f16)acc[0], (f16)acc[1]});
    o.y = as_u32(f16x2{(f16)acc[2], (f16)acc[3]});
    o.z = as_u32(f16x2{(f16)acc[4], (f16)acc[5]});
    o.w = as_u32(f16x2{(f16)acc[6], (f16)acc[7]});
    *reinterpret_cast<u32x4*>(out + (size_t)t * H + h) = o;
}

// Backward of the combine, one workgroup per token t, 256 threads x 8 columns (16-byte loads and stores):
//   dy[p][h] = fp16( fp32(dout[t][h]) * fp32(w[t][j]) )                    (torch's (dout.float() * w.float()).half())
//   dw[t][j] = sum_h fp32(dout[t][h]) * fp32(y[p][h])                      (dw may be null: no router gradient)
// for p = position[t k + j]; a slot with p = -1 writes no row and gets dw = 0.  dw's sum is a fixed tree: per thread in column
// order, then an xor butterfly per wave, then the four waves in order -- the same bits on every call.
template <typename WT>
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(const f16* __restrict__ dout, const f16* __restrict__ y,
                                                              const int* __restrict__ position, const WT* __restrict__ wts,
                                                              f16* __restrict__ dy, WT* __restrict__ dw, int k, int H)
{
    __shared__ float red[4];
    const int  t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const f16* drow = dout + (size_t)t * H;
    for (int j = 0; j < k; ++j) {
        const int p = position[(size_t)t * k + j];
        if (p < 0) {
            if (dw && tid == 0) dw[(size_t)t * k + j] = (WT)0.f;
            continue;
        }
        const float wj  = (float)wts[(size_t)t * k + j];
        float       dot = 0.f;
        for (int h = tid * 8; h < H; h += 256 * 8) {
            const f16x8 d = *reinterpret_cast<const f16x8*>(drow + h);
            f16x8       o;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                // torch's two roundings (fp32 product, then fp16): the opaque value keeps the compiler from folding the
                // multiply and the conversion into one v_fma_mix rounding, which differs in double-rounding cases
                float pr = (float)d[q] * wj;
                asm volatile("" : "+v"(pr));
                o[q] = (f16)pr;
            }
            *reinterpret_cast<f16x8*>(dy + (size_t)p * H + h) = o;
            if (dw) {
                const f16x8 v = *reinterpret_cast<const f16x8*>(y + (size_t)p * H + h);
#pragma unroll
                for (int q = 0; q < 8; ++q) dot += (float)d[q] * (float)v[q];
            }
        }
        if (dw) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
            if (lane == 0) red[wave] = dot;
            __syncthreads();
            if (tid == 0) dw[(size_t)t * k + j] = (WT)(((red[0] + red[1]) + red[2]) + red[3]);
            __syncthreads();  // red is rewritten by the next slot
        }
    }
}

// Backward of silu_mul on a glu8-ordered gate|up block: thread i owns columns 8 c .. 8 c + 7 of row r (idx =
// r I + 8 c), i.e. the 8 gate columns gu[r][16 c ..] and the 8 matching up columns gu[r][16 c + 8 ..], and writes their
// gradients to the same places of dgu:
//   du = fp16( dh * s ),  s = fp16(silu(g)) in the forward's arithmetic (so torch's grad of the fp16 multiply, bit for bit);
//   dg = fp16( fp32(dh) * fp32(u) * sig * (1 + g (1 - sig)) ),  sig = 1 / (1 + exp(-g)).
__global__ __launch_bounds__(256) void silu_mul_glu8_bwd_kernel(const f16* __restrict__ gu, const f16* __restrict__ dh,
                                                                f16* __restrict__ dgu, long rows_x_inter)
{
    const long idx = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (idx >= rows_x_inter) return;
    const f16x8 g = *reinterpret_cast<const f16x8*>(gu + 2 * idx);
    const f16x8 u = *reinterpret_cast<const f16x8*>(gu + 2 * idx + 8);
    const f16x8 d = *reinterpret_cast<const f16x8*>(dh + idx);
    f16x8       dg, du;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float x   = (float)g[q];
        const f16   s   = (f16)(x / (1.0f + expf(-x)));  // silu_mul_f16's rounded silu
        const float sig = 1.0f / (1.0f + expf(-x));
        du[q]           = d[q] * s;
        dg[q]           = (f16)((float)d[q] * (float)u[q] * sig * (1.0f + x * (1.0f - sig)));
    }
    *reinterpret_cast<f16x8*>(dgu + 2 * idx)     = dg;
    *reinterpret_cast<f16x8*>(dgu + 2 * idx + 8) = du;
}

}  // namespace

int moe_gemm_check(const char* fn, int bits, const void* x, const int8_t* w_packed, const void* scales, const int* offsets,
                   const int* sorted_slot, const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8)
{
    const std::string f(fn);
    const int         tk = bits == 4 ? gemv::Codec<4>::kTileK : kTileK;
    EETQ_REQUIRE(x && w_packed && scales && offsets && active && y && (sorted_slot || !gather), f + ": null pointer");
    EETQ_REQUIRE(E >= 1 && E <= kMoeMaxExperts, f + ": E must be in [1, 1024]");
    EETQ_REQUIRE(k >= 1 && k <= E, f + ": k must be in [1, E]");
    EETQ_REQUIRE(T >= 1 && (long long)T * k <= (1ll << 30), f + ": T must be >= 1 and T * k <= 2^30");
    EETQ_REQUIRE(N >= kTileN && N % kTileN == 0 && K >= tk && K % tk == 0,
                 f + (bits == 4 ? ": the gfx950 int4 layout needs K % 128 == 0 and N % 16 == 0"
                                : ": the gfx950 layout needs K % 64 == 0 and N % 16 == 0"));
    EETQ_REQUIRE((gather == 0 || gather == 1) && (glu8 == 0 || glu8 == 1), f + ": gather and glu8 are 0 or 1");
    EETQ_REQUIRE((long long)T * k * K < (1ll << 40) && (long long)E * K * N < (1ll << 40), f + ": activation or weight stack too large");
    EETQ_REQUIRE(aligned16(x) && aligned16(w_packed) && aligned16(y), "x, weight and y must be 16-byte aligned");
    return EETQ_OK;
}

}  // namespace eetq

using namespace eetq;

extern "C" {

int eetq_moe_route(const int64_t* top_k_index, int T, int k, int E, int* counts, int* offsets, int* sorted_slot, int* position,
                   int* active, void* stream)
{
    EETQ_REQUIRE(top_k_index && counts && offsets && sorted_slot && position && active, "eetq_moe_route: null pointer");
    EETQ_REQUIRE(E >= 1 && E <= kMoeMaxExperts, "eetq_moe_route: E must be in [1, 1024]");
    EETQ_REQUIRE(k >= 1 && k <= E, "eetq_moe_route: k must be in [1, E]");
    EETQ_REQUIRE(T >= 1 && (long long)T * k <= (1ll << 30), "eetq_moe_route: T must be >= 1 and T * k <= 2^30");
    const int    S    = T * k;
    const int    A    = S < E ? S : E;
    const size_t smem = ((size_t)kRouteWaves * E + kRouteWaves) * sizeof(int);
    if (smem > 64 * 1024) {  // E > 1023
        static std::atomic<unsigned long long> opted{0};
        int st = opt_in_large_lds(moe_route_kernel, opted);
        if (st != EETQ_OK) return st;
    }
    launch_kernel(moe_route_kernel, dim3(1), dim3(kRouteThreads), smem, static_cast<hipStream_t>(stream), top_k_index, S, E, A,
                  counts, offsets, sorted_slot, position, active);
    return check_hip(hipGetLastError(), "moe_route_kernel launch");
}

int eetq_w8a16_moe_gemm(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                        const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream)
{
    const int st = moe_gemm_check("eetq_w8a16_moe_gemm", 8, x, w_packed, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather,
                                  glu8);
    if (st != EETQ_OK) return st;
    const MoeGemmArgs a = moe_gemm_args(x, w_packed, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather, glu8, stream);
    const int         KT = K / kTileK;
    // every wave must own >= D k tiles: 8 waves from K = 1024, 4 from K = 512
    if (KT >= 16) return launch_moe_gemm_inst<8, 8, 2>(a);
    if (KT >= 8) return launch_moe_gemm_inst<8, 4, 2>(a);
    return launch_moe_gemm_inst<8, 1, 1>(a);
}

int eetq_w8a16_moe_gemm_tiled(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                              const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream)
{
    const int st = moe_gemm_check("eetq_w8a16_moe_gemm_tiled", 8, x, w_packed, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather,
                                  glu8);
    if (st != EETQ_OK) return st;
    return launch_moe_gemm_tiled(static_cast<const f16*>(x), reinterpret_cast<const uint8_t*>(w_packed), static_cast<const f16*>(scales),
                                 offsets, sorted_slot, active, static_cast<f16*>(y), T, k, E, N, K, gather != 0, glu8 != 0,
                                 static_cast<hipStream_t>(stream));
}

int eetq_w8a16_moe_gemm_tiled_supported(int T, int k, int E, int N, int K, int gather)
{
    if (T < 1 || k < 1 || E < 1 || N < 1 || K < 1) return 0;
    return moe_gemm_tiled_supports(T, k, E, N, K, gather != 0) ? 1 : 0;
}

int eetq_diag_moe_host_path(void)
{
    static const bool on = [] {
        const char* e = tuning_env("EETQ_AMD_MOE_HOST");
        return e && e[0] == '1';
    }();
    return on ? 1 : 0;
}

int eetq_moe_combine_f16(const void* y, const int* position, const void* weights, int w_dtype, void* out, int T, int k, int H,
                         void* stream)
{
    EETQ_REQUIRE(y && position && weights && out, "eetq_moe_combine_f16: null pointer");
    EETQ_REQUIRE(w_dtype == EETQ_DTYPE_F16 || w_dtype == EETQ_DTYPE_F32, "eetq_moe_combine_f16: weights must be fp16 or fp32");
    EETQ_REQUIRE(T >= 1 && k >= 1 && H >= 8 && H % 8 == 0 && (long long)T * k <= (1ll << 30),
                 "eetq_moe_combine_f16: T >= 1, k >= 1, H % 8 == 0");
    EETQ_REQUIRE(aligned16(y) && aligned16(out), "y and out must be 16-byte aligned");
    const dim3  grid((H / 8 + 255) / 256, T);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (w_dtype == EETQ_DTYPE_F32)
        launch_kernel(moe_combine_kernel<float>, grid, dim3(256), 0, s, static_cast<const f16*>(y), position,
                      static_cast<const float*>(weights), static_cast<f16*>(out), k, H);
    else
        launch_kernel(moe_combine_kernel<f16>, grid, dim3(256), 0, s, static_cast<const f16*>(y), position,
                      static_cast<const f16*>(weights), static_cast<f16*>(out), k, H);
    return check_hip(hipGetLastError(), "moe_combine_kernel launch");
}

int eetq_w8a16_moe_gemm_t(const void* dy, const int8_t* w_packed, const void* scales, const int* offsets, const int* active, void* dx,
                          int T, int k, int E, int N, int K, void* stream)
{
    EETQ_REQUIRE(dy && w_packed && scales && offsets && active && dx, "eetq_w8a16_moe_gemm_t: null pointer");
    EETQ_REQUIRE(E >= 1 && E <= kMoeMaxExperts, "eetq_w8a16_moe_gemm_t: E must be in [1, 1024]");
    EETQ_REQUIRE(k >= 1 && k <= E, "eetq_w8a16_moe_gemm_t: k must be in [1, E]");
    EETQ_REQUIRE(T >= 1 && (long long)T * k <= (1ll << 30), "eetq_w8a16_moe_gemm_t: T must be >= 1 and T * k <= 2^30");
    EETQ_REQUIRE(N >= kTileN && N % kTileN == 0 && K >= kTileK && K % kTileK == 0,
                 "eetq_w8a16_moe_gemm_t: the gfx950 layout needs K % 64 == 0 and N % 16 == 0");
    EETQ_REQUIRE((long long)T * k * (N > K ? N : K) < (1ll << 40) && (long long)E * K * N < (1ll << 40) &&
                     ((long long)T * k / 128 + E) * ((K + 127) / 128) < (1ll << 31),
                 "eetq_w8a16_moe_gemm_t: gradient or weight stack too large");
    EETQ_REQUIRE(aligned16(dy) && aligned16(w_packed) && aligned16(dx), "dy, weight and dx must be 16-byte aligned");
    return launch_moe_gemm_t(static_cast<const f16*>(dy), reinterpret_cast<const uint8_t*>(w_packed), static_cast<const f16*>(scales),
                             offsets, active, static_cast<f16*>(dx), T * k, E, N, K, static_cast<hipStream_t>(stream));
}

int eetq_moe_combine_bwd_f16(const void* dout, const void* y, const int* position, const void* weights, int w_dtype, void* dy,
                             void* dw, int T, int k, int H, void* stream)
{
    EETQ_REQUIRE(dout && y && position && weights && dy, "eetq_moe_combine_bwd_f16: null pointer");
    EETQ_REQUIRE(w_dtype == EETQ_DTYPE_F16 || w_dtype == EETQ_DTYPE_F32, "eetq_moe_combine_bwd_f16: weights must be fp16 or fp32");
    EETQ_REQUIRE(T >= 1 && k >= 1 && H >= 8 && H % 8 == 0 && (long long)T * k <= (1ll << 30),
                 "eetq_moe_combine_bwd_f16: T >= 1, k >= 1, H % 8 == 0");
    EETQ_REQUIRE(aligned16(dout) && aligned16(y) && aligned16(dy), "dout, y and dy must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (w_dtype == EETQ_DTYPE_F32)
        launch_kernel(moe_combine_bwd_kernel<float>, dim3(T), dim3(256), 0, s, static_cast<const f16*>(dout),
                      static_cast<const f16*>(y), position, static_cast<const float*>(weights), static_cast<f16*>(dy),
                      static_cast<float*>(dw), k, H);
    else
        launch_kernel(moe_combine_bwd_kernel<f16>, dim3(T), dim3(256), 0, s, static_cast<const f16*>(dout),
                      static_cast<const f16*>(y), position, static_cast<const f16*>(weights), static_cast<f16*>(dy),
                      static_cast<f16*>(dw), k, H);
    return check_hip(hipGetLastError(), "moe_combine_bwd_kernel launch");
}

int eetq_silu_mul_glu8_bwd_f16(const void* gate_up, const void* dh, void* dgate_up, int rows, int intermediate, void* stream)
{
    EETQ_REQUIRE(gate_up && dh && dgate_up, "eetq_silu_mul_glu8_bwd_f16: null pointer");
    EETQ_REQUIRE(rows >= 1 && intermediate >= 8 && intermediate % 8 == 0, "eetq_silu_mul_glu8_bwd_f16: rows >= 1, I % 8 == 0");
    EETQ_REQUIRE(aligned16(gate_up) && aligned16(dh) && aligned16(dgate_up), "gate_up, dh and dgate_up must be 16-byte aligned");
    const long n = (long)rows * intermediate;
    launch_kernel(silu_mul_glu8_bwd_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                  static_cast<const f16*>(gate_up), static_cast<const f16*>(dh), static_cast<f16*>(dgate_up), n);
    return check_hip(hipGetLastError(), "silu_mul_glu8_bwd_kernel launch");
}

}  // extern "C"
