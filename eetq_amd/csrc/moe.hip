// Routed mixture-of-experts kernels: device-side routing tables, the grouped W8A16 GEMM over an [E][K][N] int8
// expert stack that reads them, and the weighted combine; and the backward's combine and gated-activation steps (DESIGN.md 4.11,
// whose grouped input-gradient GEMM lives in gemm_t.hip).  No launch needs a host sync, so a decode step's MoE layer
// (route -> gate|up GEMM with the gated activation -> down GEMM -> combine) can be captured in a graph; the grid of every launch
// depends on T, k, E, N and K only, never on the routing.
#include "common.hpp"
#include "gemv_kernel.hpp"

namespace eetq {

namespace {

constexpr int kRouteThreads = 1024;  // 16 waves; wave w owns the w-th contiguous segment of the T*k slots
constexpr int kRouteWaves   = kRouteThreads / 64;
constexpr int kMoeMaxExperts = 1024;

// exclusive block-wide prefix sum of v (every thread of the kRouteThreads calls it); *total = the sum over the block.
// wsum: kRouteWaves ints of LDS.  Deterministic: a fixed tree of integer adds.
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int       inc  = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kRouteWaves; ++w) {
        const int s = wsum[w];
        base += w < wave ? s : 0;
        all += s;
    }
    __syncthreads();  // wsum is reused by the next call
    *total = all;
    return base + inc - v;
}

// the lanes of this wave whose expert id equals mine (ids < 2^nbits; invalid lanes pass id = -1 and get an empty mask)
__device__ __forceinline__ unsigned long long same_id_lanes(int id, int nbits)
{
    unsigned long long m = __ballot(id >= 0);
    for (int b = 0; b < nbits; ++b) {
        const unsigned long long set = __ballot(id >= 0 && ((id >> b) & 1));
        m &= ((id >> b) & 1) ? set : ~set;
    }
    return id >= 0 ? m : 0ull;
}

// One workgroup.  Dynamic LDS: kRouteWaves * E ints (per-wave, per-expert counters) + kRouteWaves ints (scan).
// Pass 1: wave w counts the ids of its slot segment (the lowest lane of every group of equal ids adds the group's size).
// Scan:   counts, offsets, the active list; every per-wave counter becomes that wave's first position for the expert.
// Pass 2: wave w walks its segment again in the same order: position = its counter + the rank among equal ids of lower lanes.
// Segments are in slot order and so are lanes within a chunk: sorted_slot is ordered by expert, then by slot, whatever the timing.
__global__ __launch_bounds__(kRouteThreads) void moe_route_kernel(const int64_t* __restrict__ idx, int S, int E, int A,
                                                                   int* __restrict__ counts, int* __restrict__ offsets,
                                                                   int* __restrict__ sorted_slot, int* __restrict__ position,
                                                                   int* __restrict__ active)
{
    extern __shared__ int lds[];
    int*      cnt  = lds;                     // [kRouteWaves][E]
    int*      wsum = lds + kRouteWaves * E;   // [kRouteWaves]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbits = 32 - __clz(E - 1 > 0 ? E - 1 : 1);
    for (int i = tid; i < kRouteWaves * E; i += kRouteThreads) cnt[i] = 0;
    __syncthreads();

    const int seg = (S + kRouteWaves - 1) / kRouteWaves;
    const int s0 = wave * seg, s1 = min(S, s0 + seg);
    int*      mine = cnt + wave * E;
    for (int c = s0; c < s1; c += 64) {
        const int     s  = c + lane;
        const int64_t v  = s < s1 ? idx[s] : -1;
        const int     id = (v >= 0 && v < E) ? (int)v : -1;
        const unsigned long long m = same_id_lanes(id, nbits);
        if (id >= 0 && (m & ((1ull << lane) - 1)) == 0) mine[id] += __popcll(m);
    }
    __syncthreads();

    int carry = 0, carry_active = 0;
    for (int e0 = 0; e0 < E; e0 += kRouteThreads) {
        const int e = e0 + tid;
        int       n = 0;
        if (e < E)
            for (int w = 0; w < kRouteWaves; ++w) n += cnt[w * E + e];
        int       tot_n, tot_a;
        const int off = carry + block_excl_scan(n, wsum, &tot_n);
        const int act = carry_active + block_excl_scan(n > 0 ? 1 : 0, wsum, &tot_a);
        if (e < E) {
            counts[e]  = n;
            offsets[e] = off;
            if (n > 0) active[act] = e;
            int base = off;
            for (int w = 0; w < kRouteWaves; ++w) {
                const int c = cnt[w * E + e];
                cnt[w * E + e] = base;
                base += c;
            }
        }
        carry += tot_n;
        carry_active += tot_a;
    }
    if (tid == 0) offsets[E] = carry;
    for (int a = carry_active + tid; a < A; a += kRouteThreads) active[a] = -1;
    for (int s = carry + tid; s < S; s += kRouteThreads) sorted_slot[s] = -1;
    __syncthreads();

    for (int c = s0; c < s1; c += 64) {
        const int     s  = c + lane;
        const int64_t v  = s < s1 ? idx[s] : -1;
        const int     id = (v >= 0 && v < E) ? (int)v : -1;
        const unsigned long long m = same_id_lanes(id, nbits);
        const unsigned long long below = m & ((1ull << lane) - 1);
        int pos = -1;
        if (id >= 0) pos = mine[id] + __popcll(below);  // every lane reads before the group's lowest lane moves the counter on
        if (id >= 0) sorted_slot[pos] = s;
        if (s < s1) position[s] = pos;
        if (id >= 0 && below == 0) mine[id] += __popcll(m);
    }
}

// Grouped GEMM over the expert stack: the small-batch stream kernel's body (streamk_kernel.hpp, one row tile, activations straight
// from global memory: XM = 0, int8) with a row map.  blockIdx.y = active slot a (exit on -1), blockIdx.x = 16-column tile row.
// Rows of expert e: sorted positions offsets[e] .. offsets[e + 1] - 1, taken 16 at a time (one MFMA row tile; T <= 16 needs one).
// Row p reads x[sorted_slot[p] / k] (GATHER) or x[p], and writes y[p].  The expert's weight tile row is streamed once per 16 rows.
// GLU8: columns in glu8 order (8 gate + the matching 8 up per 16-column tile), y[p][8 tile + c] = silu_mul(gate, up) -- the
// streamk kernel's glu8 epilogue, i.e. the projection followed by eetq_silu_mul_glu8_f16, bit for bit.
template <int WAVES, int D, bool GATHER, bool GLU8>
__global__ __launch_bounds__(WAVES * 64) void moe_gemm_kernel(const f16* __restrict__ x, const uint8_t* __restrict__ w_all,
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
    const int KT    = K / kTileK;
    const int ntile = blockIdx.x;

    const uint8_t* w      = w_all + (size_t)e * K * N;
    const f16*     scales = scales_all + (size_t)e * N;
    const u32      sraw   = reinterpret_cast<const uint16_t*>(scales)[ntile * 16 + c];
    const u32x4*   wp     = reinterpret_cast<const u32x4*>(w + (size_t)ntile * KT * kTileBytes) + lane;  // + 64 per k tile

    for (int r0 = 0; r0 < rows; r0 += 16) {
        // lane (g, c) feeds row r0 + c (clamped: rows beyond the expert's compute garbage that is never stored)
        const int rc = r0 + c < rows ? r0 + c : rows - 1;
        const int xr = GATHER ? sorted_slot[p0 + rc] / topk : p0 + rc;
        const u32x4* xrow = reinterpret_cast<const u32x4*>(x + (size_t)xr * K + 16 * g);  // + 8 u32x4 per k tile

        struct Stage {
            u32x4 wq, xa[2];
        };
        auto load_stage = [&](int kt, Stage& s) {
            s.wq    = gemv::load_w<true>(wp + (size_t)kt * 64);
            s.xa[0] = xrow[(size_t)kt * 8];
            s.xa[1] = xrow[(size_t)kt * 8 + 1];
        };
        f32x4       acc    = {0.f, 0.f, 0.f, 0.f};
        const f16x2 scale2 = as_f16x2(sraw | (sraw << 16));
        auto consume = [&](const Stage& s) {
            f16x2 wq[8];
            dequant_16(s.wq, scale2, wq);
            const f16x8 b0 = {wq[0].x, wq[0].y, wq[1].x, wq[1].y, wq[2].x, wq[2].y, wq[3].x, wq[3].y};
            const f16x8 b1 = {wq[4].x, wq[4].y, wq[5].x, wq[5].y, wq[6].x, wq[6].y, wq[7].x, wq[7].y};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, s.xa[0]), b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, s.xa[1]), b1, acc, 0, 0, 0);
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

template <int WAVES, int D>
int launch_moe_gemm_inst(const f16* x, const uint8_t* w, const f16* s, const int* offsets, const int* sorted_slot,
                         const int* active, f16* y, int topk, int A, int N, int K, bool gather, bool glu8, hipStream_t stream)
{
    const dim3 grid(N / kTileN, A), block(WAVES * 64);
    if (gather)
        glu8 ? launch_kernel(moe_gemm_kernel<WAVES, D, true, true>, grid, block, 0, stream, x, w, s, offsets, sorted_slot, active, y, topk, N, K)
             : launch_kernel(moe_gemm_kernel<WAVES, D, true, false>, grid, block, 0, stream, x, w, s, offsets, sorted_slot, active, y, topk, N, K);
    else
        glu8 ? launch_kernel(moe_gemm_kernel<WAVES, D, false, true>, grid, block, 0, stream, x, w, s, offsets, sorted_slot, active, y, topk, N, K)
             : launch_kernel(moe_gemm_kernel<WAVES, D, false, false>, grid, block, 0, stream, x, w, s, offsets, sorted_slot, active, y, topk, N, K);
    return check_hip(hipGetLastError(), "moe_gemm_kernel launch");
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

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// the argument checks eetq_w8a16_moe_gemm and eetq_w8a16_moe_gemm_tiled share (`fn` names the entry in the messages)
int moe_gemm_check(const char* fn, const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                   const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8)
{
    const std::string f(fn);
    EETQ_REQUIRE(x && w_packed && scales && offsets && active && y && (sorted_slot || !gather), f + ": null pointer");
    EETQ_REQUIRE(E >= 1 && E <= kMoeMaxExperts, f + ": E must be in [1, 1024]");
    EETQ_REQUIRE(k >= 1 && k <= E, f + ": k must be in [1, E]");
    EETQ_REQUIRE(T >= 1 && (long long)T * k <= (1ll << 30), f + ": T must be >= 1 and T * k <= 2^30");
    EETQ_REQUIRE(N >= kTileN && N % kTileN == 0 && K >= kTileK && K % kTileK == 0,
                 f + ": the gfx950 layout needs K % 64 == 0 and N % 16 == 0");
    EETQ_REQUIRE((gather == 0 || gather == 1) && (glu8 == 0 || glu8 == 1), f + ": gather and glu8 are 0 or 1");
    EETQ_REQUIRE((long long)T * k * K < (1ll << 40) && (long long)E * K * N < (1ll << 40), f + ": activation or weight stack too large");
    EETQ_REQUIRE(aligned16(x) && aligned16(w_packed) && aligned16(y), "x, weight and y must be 16-byte aligned");
    return EETQ_OK;
}

}  // namespace

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
    const int st = moe_gemm_check("eetq_w8a16_moe_gemm", x, w_packed, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather, glu8);
    if (st != EETQ_OK) return st;
    const int   S  = T * k;
    const int   A  = S < E ? S : E;
    const int   KT = K / kTileK;
    const auto  xp = static_cast<const f16*>(x);
    const auto  wp = reinterpret_cast<const uint8_t*>(w_packed);
    const auto  sp = static_cast<const f16*>(scales);
    const auto  yp = static_cast<f16*>(y);
    hipStream_t s  = static_cast<hipStream_t>(stream);
    const bool  g = gather != 0, a = glu8 != 0;
    // every wave must own >= D k tiles: 8 waves from K = 1024, 4 from K = 512
    if (KT >= 16) return launch_moe_gemm_inst<8, 2>(xp, wp, sp, offsets, sorted_slot, active, yp, k, A, N, K, g, a, s);
    if (KT >= 8) return launch_moe_gemm_inst<4, 2>(xp, wp, sp, offsets, sorted_slot, active, yp, k, A, N, K, g, a, s);
    return launch_moe_gemm_inst<1, 1>(xp, wp, sp, offsets, sorted_slot, active, yp, k, A, N, K, g, a, s);
}

int eetq_w8a16_moe_gemm_tiled(const void* x, const int8_t* w_packed, const void* scales, const int* offsets, const int* sorted_slot,
                              const int* active, void* y, int T, int k, int E, int N, int K, int gather, int glu8, void* stream)
{
    const int st = moe_gemm_check("eetq_w8a16_moe_gemm_tiled", x, w_packed, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather, glu8);
    if (st != EETQ_OK) return st;
    return launch_moe_gemm_tiled(static_cast<const f16*>(x), reinterpret_cast<const uint8_t*>(w_packed), static_cast<const f16*>(scales),
                                 offsets, sorted_slot, active, static_cast<f16*>(y), T, k, E, N, K, gather != 0, glu8 != 0,
                                 static_cast<hipStream_t>(stream));
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
