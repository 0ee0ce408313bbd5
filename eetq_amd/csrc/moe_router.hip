// The mixture-of-experts router on the device: what transformers' *TopKRouter modules compute -- F.linear ->
// softmax(float) -> topk -> renormalise -- and the routing tables of eetq_moe_route for the indices it selects.
//   T <= 16: ONE launch.  The router weight (up to 512 KiB) is streamed by many workgroups, each owning a few experts' rows; they
//            hand their fp32 logits to whichever workgroup finishes last, which rounds them, selects, scores and builds the tables.
//   T  > 16: the same logits kernel per 16-token chunk (no hand-over), the selection kernel, eetq_moe_route.
// The hand-over is the split-K kernel's (gemm_splitk_kernel.hpp): write-through stores, every storing wave drains them, a
// workgroup barrier, one lane takes an agent-scope ticket, the last arriver reads everything back with loads that bypass its L1.
// No float atomics; the result bits do not depend on which workgroup finishes.
// The same kernels carry a second routing rule: DeepSeek-V3's sigmoid scores with a correction bias and group-limited
// selection, on fp32 logits (kSigmoid instantiations; the softmax instantiations are the code they were before).
#include <mutex>
#include <type_traits>

#include "moe_route_tables.hpp"

namespace eetq {

namespace {

constexpr int kRouterThreads = 256;  // 4 waves
constexpr int kRouterWaves   = kRouterThreads / 64;
constexpr int kRouterMaxE    = 256;  // 4 logits per lane in the selection
constexpr int kRouterMaxK    = 16;
constexpr int kRouterTokens  = 16;   // tokens per logits workgroup: the fused launch's T limit, the chunk above it
constexpr int kSlabStride    = 32;   // floats per expert in the hand-over slab: one 128-byte line each, written by one store
constexpr int kSlabFloats    = kRouterMaxE * kSlabStride;

// LDS of the logits kernel (bytes): cross-wave sums | ticket | selected ids | route counters + scan | fp16 logits
constexpr int kLdsRed  = 0;
constexpr int kLdsFlag = kLdsRed + kRouterWaves * kRouterTokens * 4;
constexpr int kLdsIdx  = kLdsFlag + 16;
constexpr int kLdsCnt  = kLdsIdx + kRouterTokens * kRouterMaxK * 4;
constexpr int kLdsLog  = kLdsCnt + kRouterWaves * kRouterMaxE * 4 + 16;  // route_tables: [waves][E] counters + [waves] scan
constexpr int kLdsUsed = kLdsLog + kRouterTokens * kRouterMaxE * 2;
// the sigmoid rule's finish keeps fp32 logits (16 KiB instead of 8) and, per wave, one row of scores for choice and one of sigmoids
constexpr int kLdsSig     = kLdsLog + kRouterTokens * kRouterMaxE * 4;
constexpr int kLdsSigUsed = kLdsSig + kRouterWaves * 2 * kRouterMaxE * 4;
// the fused launch asks for more than half a CU's LDS, so at most one of its workgroups is resident per CU: the occupancy the
// write-through hand-over has been measured at
constexpr int kLdsFused = 84 * 1024;
static_assert(kLdsSigUsed <= kLdsFused, "the sigmoid rule's finish fits the fused launch's LDS");
constexpr int kRouterMaxG = 64;  // one lane per group

// the sigmoid rule's arguments, passed to the kernels by value
struct SigmoidRule {
    const void* bias;        // e_score_correction_bias [E], fp16 or fp32
    int         bias_dtype;  // EETQ_DTYPE_F16 / EETQ_DTYPE_F32
    int         n_group, topk_group;
    float       scale;       // routed_scaling_factor
};

typedef __attribute__((address_space(1))) unsigned gu32;

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// ---- selection and scores: ONE wave per token, shared by both kernels (same logits in, same bits out) ------------------------
// A logit and its expert id as one key whose unsigned order is (larger logit, then lower id); 0 is below every valid key.
__device__ __forceinline__ u32 logit_key(f16 v, int e)
{
    u32 b = __builtin_bit_cast(unsigned short, v);
    if (b == 0x8000u) b = 0;  // -0 ties with +0
    const u32 o = (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
    return (o << 16) | (0xffffu - (u32)e);
}
__device__ __forceinline__ float key_logit(u32 key)
{
    const u32            o = key >> 16;
    const unsigned short b = (unsigned short)((o & 0x8000u) ? (o ^ 0x8000u) : (~o & 0xffffu));
    return (float)__builtin_bit_cast(f16, b);
}

// logit(e) = the token's fp16 logit of expert e < E <= 256.  Lane j < k ends up with the j-th choice:
//   id_j    = the j-th largest logit's expert, ties to the lower id;
//   p_j     = exp(l_j - max) / sum_e exp(l_e - max) in fp32 (the sum: per lane in expert order, then an xor butterfly);
//   renorm: p_j / (p_0 + p_1 + ... + p_{k-1}), summed in that order.
// idx_out [k] int64, w_out [k] of w_dtype, idx_lds (may be null) [k] int.
template <typename LoadFn>
__device__ __forceinline__ void router_select_wave(LoadFn logit, int E, int k, int renorm, int w_dtype, int64_t* idx_out, void* w_out,
                                                   int* idx_lds)
{
    const int lane = threadIdx.x & 63;
    u32       key[4];
    float     val[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = lane + 64 * q;
        const f16 v = e < E ? logit(e) : (f16)0.f;
        key[q]      = e < E ? logit_key(v, e) : 0u;
        val[q]      = (float)v;
    }
    int   my_id = 0;
    float my_l = 0.f, top = 0.f;
    for (int j = 0; j < k; ++j) {
        u32 best = max(max(key[0], key[1]), max(key[2], key[3]));
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) best = max(best, (u32)__shfl_xor((int)best, m, 64));
#pragma unroll
        for (int q = 0; q < 4; ++q) key[q] = key[q] == best ? 0u : key[q];  // keys are unique: exactly one lane drops one
        const float l = key_logit(best);
        if (j == 0) top = l;
        if (lane == j) {
            my_id = (int)(0xffffu - (best & 0xffffu));
            my_l  = l;
        }
    }
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) sum += lane + 64 * q < E ? expf(val[q] - top) : 0.f;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    float p = lane < k ? expf(my_l - top) / sum : 0.f;
    if (renorm) {
        float tot = 0.f;
        for (int j = 0; j < k; ++j) tot += __shfl(p, j, 64);
        p = p / tot;
    }
    if (lane < k) {
        idx_out[lane] = my_id;
        if (idx_lds) idx_lds[lane] = my_id;
        if (w_dtype == EETQ_DTYPE_F32) static_cast<float*>(w_out)[lane] = p;
        else static_cast<f16*>(w_out)[lane] = (f16)p;
    }
}

// ---- the sigmoid, bias-corrected, group-limited rule: ONE wave per token, shared by both kernels ----------------
// An fp32 value and an id < 2^32 as one key whose unsigned order is (larger value, then lower id); 0 is below every valid key.
__device__ __forceinline__ unsigned long long score_key(float v, int id)
{
    u32 b = __builtin_bit_cast(u32, v);
    if (b == 0x80000000u) b = 0;  // -0 ties with +0
    const u32 o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)o << 32) | (0xffffffffu - (u32)id);
}
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// logit(e) = the token's fp32 logit of expert e < E <= 256; rows = this wave's LDS [2][256] floats.  Lane j < k ends up with choice j:
//   s_e = 1 / (1 + exp(-logit_e)), c_e = s_e + bias_e in fp32;
//   group g < G (E / G contiguous experts) scores the sum of its two largest c; the KG best groups stay, ties to the lower group;
//   id_j = the j-th largest c among the experts of those groups, ties to the lower id;
//   wgt_j = s[id_j]; renorm: wgt_j / (wgt_0 + ... + wgt_{k-1} + 1e-20), summed in that order; then * scale.
// The caller guarantees k <= KG * E / G (every choice has a valid key).  idx_out, w_out, idx_lds as router_select_wave.
template <typename LoadFn>
__device__ __forceinline__ void router_select_sigmoid_wave(LoadFn logit, const SigmoidRule& r, int E, int k, int renorm, int w_dtype,
                                                           int64_t* idx_out, void* w_out, int* idx_lds, float* rows)
{
    const int lane = threadIdx.x & 63;
    float*    crow = rows;
    float*    srow = rows + kRouterMaxE;
    float     c[4];
    __builtin_amdgcn_wave_barrier();  // the previous token's reads of the rows are issued
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = lane + 64 * q;
        c[q]        = 0.f;
        if (e < E) {
            const float s = 1.f / (1.f + expf(-logit(e)));
            const float b = r.bias_dtype == EETQ_DTYPE_F32 ? static_cast<const float*>(r.bias)[e]
                                                           : (float)static_cast<const f16*>(r.bias)[e];
            c[q]    = s + b;
            crow[e] = c[q];
            srow[e] = s;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int G = r.n_group, per = E / G;
    unsigned long long kept = 1ull;  // bit g: group g stays
    if (G > 1) {
        unsigned long long gkey = 0;
        if (lane < G) {
            const float* grp = crow + lane * per;
            float        m1 = grp[0], m2 = grp[1];
            if (m2 > m1) {
                const float t = m1;
                m1 = m2;
                m2 = t;
            }
            for (int i = 2; i < per; ++i) {
                const float v = grp[i];
                m2 = v > m1 ? m1 : (v > m2 ? v : m2);
                m1 = v > m1 ? v : m1;
            }
            gkey = score_key(m1 + m2, lane);
        }
        bool mine = false;
        for (int j = 0; j < r.topk_group; ++j) {
            const unsigned long long best = wave_max_key(gkey);
            if (gkey == best) {  // keys are unique: exactly one lane
                mine = true;
                gkey = 0;
            }
        }
        kept = __ballot(mine);
    }
    unsigned long long key[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = lane + 64 * q;
        key[q]      = (e < E && ((kept >> (e / per)) & 1ull)) ? score_key(c[q], e) : 0ull;
    }
    int my_id = 0;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = key[0] > key[1] ? key[0] : key[1];
        const unsigned long long b23 = key[2] > key[3] ? key[2] : key[3];
        best = wave_max_key(b23 > best ? b23 : best);
#pragma unroll
        for (int q = 0; q < 4; ++q) key[q] = key[q] == best ? 0ull : key[q];
        if (lane == j) my_id = (int)(0xffffffffu - (u32)best);
    }
    float p = lane < k ? srow[my_id] : 0.f;
    if (renorm) {
        float tot = 0.f;
        for (int j = 0; j < k; ++j) tot += __shfl(p, j, 64);
        p = p / (tot + 1e-20f);
    }
    p *= r.scale;
    if (lane < k) {
        idx_out[lane] = my_id;
        if (idx_lds) idx_lds[lane] = my_id;
        if (w_dtype == EETQ_DTYPE_F32) static_cast<float*>(w_out)[lane] = p;
        else static_cast<f16*>(w_out)[lane] = (f16)p;
    }
}

// ---- logits (+ the fused finish) ----------------------------------------------------------------------------------------------
// grid (G, chunks), 256 threads.  Workgroup (g, c): experts g * epw .. + epw - 1 (epw = 4 / wpe), tokens 16 c .. 16 c + 15; wave v
// owns expert v / wpe's columns [(v % wpe) H / wpe, +H / wpe): each lane keeps 8 weight columns in registers per step and walks the
// tokens.  sum = fixed order: per lane along H, an xor butterfly over the wave, the wpe waves in order; logit = fp16(sum).
//   ticket == null (chunked): the logits are stored and the workgroup is done.
//   ticket != null (fused, one chunk): the fp32 sums go to `slab` [E][32] write-through, and the last workgroup to arrive finishes.
// kSigmoid: the logits stay fp32 (`logits` is float [T][E], the sum unrounded) and the finish is the sigmoid rule `rule`; otherwise
// `logits` is f16 [T][E] and `rule` is not read.
template <bool kSigmoid>
__global__ __launch_bounds__(kRouterThreads) void moe_router_kernel(const f16* __restrict__ x, const f16* __restrict__ w, int T, int H,
                                                                    int E, int k, int renorm, int w_dtype, int wpe, void* logits_out,
                                                                    int64_t* top_k_index, void* top_k_weights, int* counts, int* offsets,
                                                                    int* sorted_slot, int* position, int* active, float* slab,
                                                                    unsigned* ticket, SigmoidRule rule)
{
    typedef typename std::conditional<kSigmoid, float, f16>::type logit_t;
    logit_t* logits = static_cast<logit_t*>(logits_out);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float*    red  = reinterpret_cast<float*>(smem + kLdsRed);      // [waves][16]
    unsigned* flag = reinterpret_cast<unsigned*>(smem + kLdsFlag);
    int*      sidx = reinterpret_cast<int*>(smem + kLdsIdx);        // [T][k]
    int*      cnt  = reinterpret_cast<int*>(smem + kLdsCnt);        // route_tables' [waves][E] + [waves]
    logit_t*  slog = reinterpret_cast<logit_t*>(smem + kLdsLog);    // [T][E]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int epw = kRouterWaves / wpe;
    const int e   = blockIdx.x * epw + wave / wpe;
    const int hs  = H / wpe, h0 = (wave % wpe) * hs;
    const int t0  = blockIdx.y * kRouterTokens;
    const int Tc  = min(kRouterTokens, T - t0);

    float acc[kRouterTokens];
#pragma unroll
    for (int t = 0; t < kRouterTokens; ++t) acc[t] = 0.f;
    if (e < E) {
        const f16* wr = w + (size_t)e * H + h0;
        const f16* xr = x + (size_t)t0 * H + h0;
        // memory-level parallelism: the next step's weight is in flight while this step computes, and the x rows come four at a
        // time, all four loads issued before the first use (row index clamped to the chunk: a row past Tc re-reads the last one
        // into an accumulator nobody reads), behind one uniform branch per four tokens
        int   h  = lane * 8;
        f16x8 wv = *reinterpret_cast<const f16x8*>(wr + (h < hs ? h : 0));
        for (; h < hs; h += 512) {
            const f16x8 wn = *reinterpret_cast<const f16x8*>(wr + (h + 512 < hs ? h + 512 : h));
#pragma unroll
            for (int g = 0; g < kRouterTokens / 4; ++g)
                if (4 * g < Tc) {
                    f16x8 xv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        xv[i] = *reinterpret_cast<const f16x8*>(xr + (size_t)min(4 * g + i, Tc - 1) * H + h);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < 8; ++q) acc[4 * g + i] += (float)xv[i][q] * (float)wv[q];
                }
            wv = wn;
        }
    }
    float mine = 0.f;  // lane t < 16 keeps token t's sum over this wave's columns
#pragma unroll
    for (int t = 0; t < kRouterTokens; ++t) {
        float s = acc[t];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        mine = lane == t ? s : mine;
    }
    if (lane < kRouterTokens) red[wave * kRouterTokens + lane] = mine;
    __syncthreads();

    const bool fused = ticket != nullptr;
    if (tid < epw * kRouterTokens) {
        const int es = tid >> 4, t = tid & 15, ee = blockIdx.x * epw + es;
        float     s  = 0.f;
        for (int q = 0; q < wpe; ++q) s += red[(es * wpe + q) * kRouterTokens + t];
        if (t < Tc && ee < E) {
            if (fused)  // write-through, 4 bytes per lane, one 128-byte line per expert
                __hip_atomic_store(((gu32*)slab) + ee * kSlabStride + t, __builtin_bit_cast(u32, s), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            else
                logits[(size_t)(t0 + t) * E + ee] = (logit_t)s;
        }
    }
    if (!fused) return;

    // ---- hand-over: every storing wave drains, the workgroup meets, one lane takes the ticket ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) *flag = __hip_atomic_fetch_add(((gu32*)ticket), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != gridDim.x - 1) return;
    // ---- last arriver: the ticket goes back to 0 for the stream's next launch; all sums read back below this CU's L1 ----
    if (tid == 0) __hip_atomic_store(((gu32*)ticket), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = tid; i < T * E; i += kRouterThreads) {
        const int t = i / E, ee = i - t * E;
        const u32 v = __hip_atomic_load(((gu32*)slab) + ee * kSlabStride + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const logit_t l = (logit_t)__builtin_bit_cast(float, v);
        slog[i]         = l;
        logits[i]       = l;
    }
    __syncthreads();
    const bool tables = counts != nullptr;
    const int  wbytes = w_dtype == EETQ_DTYPE_F32 ? 4 : 2;
    for (int t = wave; t < T; t += kRouterWaves) {
        const logit_t* row  = slog + t * E;
        int64_t*       io   = top_k_index + (size_t)t * k;
        void*          wo   = static_cast<char*>(top_k_weights) + (size_t)t * k * wbytes;
        int*           il   = tables ? sidx + t * k : nullptr;
        const auto     load = [row](int ee) { return row[ee]; };
        if constexpr (kSigmoid)
            router_select_sigmoid_wave(load, rule, E, k, renorm, w_dtype, io, wo, il,
                                       reinterpret_cast<float*>(smem + kLdsSig) + wave * 2 * kRouterMaxE);
        else
            router_select_wave(load, E, k, renorm, w_dtype, io, wo, il);
    }
    if (!tables) return;
    __syncthreads();
    const int S = T * k;
    route_tables<kRouterThreads>([sidx](int s) { return (int64_t)sidx[s]; }, S, E, S < E ? S : E, cnt, counts, offsets,
                                 sorted_slot, position, active);
}

// the selection on its own: grid ceil(T / 4), one wave per token
__global__ __launch_bounds__(kRouterThreads) void moe_topk_kernel(const f16* __restrict__ logits, int T, int E, int k, int renorm,
                                                                  int w_dtype, int64_t* __restrict__ top_k_index,
                                                                  void* __restrict__ top_k_weights)
{
    const int t = blockIdx.x * kRouterWaves + (threadIdx.x >> 6);
    if (t >= T) return;
    const f16* row    = logits + (size_t)t * E;
    const int  wbytes = w_dtype == EETQ_DTYPE_F32 ? 4 : 2;
    router_select_wave([row](int ee) { return row[ee]; }, E, k, renorm, w_dtype, top_k_index + (size_t)t * k,
                       static_cast<char*>(top_k_weights) + (size_t)t * k * wbytes, nullptr);
}

// the sigmoid rule's selection on its own, from fp32 logits: grid ceil(T / 4), one wave per token
__global__ __launch_bounds__(kRouterThreads) void moe_topk_sigmoid_kernel(const float* __restrict__ logits, int T, int E, int k, int renorm,
                                                                          int w_dtype, int64_t* __restrict__ top_k_index,
                                                                          void* __restrict__ top_k_weights, SigmoidRule rule)
{
    __shared__ float rows[kRouterWaves][2 * kRouterMaxE];
    const int wave = threadIdx.x >> 6;
    const int t    = blockIdx.x * kRouterWaves + wave;
    if (t >= T) return;
    const float* row    = logits + (size_t)t * E;
    const int    wbytes = w_dtype == EETQ_DTYPE_F32 ? 4 : 2;
    router_select_sigmoid_wave([row](int ee) { return row[ee]; }, rule, E, k, renorm, w_dtype, top_k_index + (size_t)t * k,
                               static_cast<char*>(top_k_weights) + (size_t)t * k * wbytes, nullptr, rows[wave]);
}

// ---- the hand-over scratch: one ticket line + one slab per launch stream ----------------------------------------------------------
// Per device one allocation, made by the first fused launch (never during a graph capture): kSlots ticket lines (128 bytes each,
// zero; the finishing workgroup of every launch puts its ticket back to 0) followed by kSlots slabs of 32 KiB.  A slot belongs to
// the stream that first launched with it, for good: launches of one stream are ordered, so they never share a slot in flight, and a
// captured graph replays with the slot of its capture stream.  Freed by eetq_release_workspace().
constexpr int    kSlots      = 64;
constexpr size_t kTicketLine = 128;
constexpr size_t kArenaBytes = kSlots * (kTicketLine + kSlabFloats * sizeof(float));

struct Arena {
    uint8_t*    base = nullptr;
    hipStream_t owner[kSlots];
    int         used = 0;
};
std::mutex g_mutex;
Arena      g_arena[64];

int slot_for(hipStream_t stream, float** slab, unsigned** ticket)
{
    int dev = 0;
    EETQ_TRY_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_mutex);
    Arena& a = g_arena[dev & 63];
    if (!a.base) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return fail(EETQ_ERR_UNSUPPORTED,
                        "[eetq_amd] eetq_moe_router_f16: the hand-over scratch cannot be created during a graph capture; run the "
                        "router once (T <= 16) on this device before capturing");
        uint8_t* p = nullptr;
        EETQ_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&p), kArenaBytes));
        hipError_t e = hipMemset(p, 0, kSlots * kTicketLine);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) {
            (void)hipFree(p);
            return check_hip(e, "moe router scratch");
        }
        a.base = p;
        a.used = 0;
    }
    int s = 0;
    while (s < a.used && a.owner[s] != stream) ++s;
    if (s == a.used) {
        if (a.used == kSlots)
            return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] eetq_moe_router_f16: more than 64 launch streams on one device; "
                                              "eetq_release_workspace() frees their slots");
        a.owner[a.used++] = stream;
    }
    *ticket = reinterpret_cast<unsigned*>(a.base + s * kTicketLine);
    *slab   = reinterpret_cast<float*>(a.base + kSlots * kTicketLine) + (size_t)s * kSlabFloats;
    return EETQ_OK;
}

// waves per expert: as many as have at least one full 512-column step of the row each (1, 2 or 4)
int waves_per_expert(int H) { return H >= 2048 ? 4 : (H >= 1024 ? 2 : 1); }

int check_select(const std::string& f, int T, int E, int k, int renorm, int w_dtype)
{
    EETQ_REQUIRE(E >= 1, f + ": E must be >= 1");
    EETQ_REQUIRE(k >= 1 && k <= E, f + ": k must be in [1, E]");
    if (E > kRouterMaxE || k > kRouterMaxK) return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] " + f + ": E <= 256 and k <= 16 are served");
    EETQ_REQUIRE(T >= 1 && (long long)T * E < (1ll << 31), f + ": T must be >= 1 and T * E < 2^31");
    EETQ_REQUIRE(renorm == 0 || renorm == 1, f + ": renorm is 0 or 1");
    EETQ_REQUIRE(w_dtype == EETQ_DTYPE_F16 || w_dtype == EETQ_DTYPE_F32, f + ": the scores must be fp16 or fp32");
    return EETQ_OK;
}

// the sigmoid rule's own limits, after check_select
int check_sigmoid(const std::string& f, const void* bias, int bias_dtype, int E, int k, int n_group, int topk_group, float scale)
{
    EETQ_REQUIRE(bias != nullptr, f + ": null pointer");
    EETQ_REQUIRE(bias_dtype == EETQ_DTYPE_F16 || bias_dtype == EETQ_DTYPE_F32, f + ": the bias must be fp16 or fp32");
    EETQ_REQUIRE(n_group >= 1, f + ": n_group must be >= 1");
    if (n_group > kRouterMaxG) return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] " + f + ": n_group <= 64 is served");
    EETQ_REQUIRE(E % n_group == 0, f + ": E must be a multiple of n_group");
    EETQ_REQUIRE(n_group == 1 || E / n_group >= 2, f + ": a group needs at least two experts (its score is the sum of its two best)");
    EETQ_REQUIRE(topk_group >= 1 && topk_group <= n_group, f + ": topk_group must be in [1, n_group]");
    EETQ_REQUIRE(k <= topk_group * (E / n_group), f + ": k must not exceed the experts of the topk_group kept groups");
    EETQ_REQUIRE(scale == scale && scale - scale == 0.f, f + ": routed_scaling_factor must be finite");
    return EETQ_OK;
}

// Both routing rules' entry: rule == null is the softmax router on fp16 logits, else the sigmoid rule on fp32 logits.
int router_entry(const char* fn, const void* x, const void* w, const SigmoidRule* rule, int T, int H, int E, int k, int renorm, int w_dtype,
                 void* logits_out, int64_t* top_k_index, void* top_k_weights, int* counts, int* offsets, int* sorted_slot, int* position,
                 int* active, void* stream)
{
    const std::string f = fn;
    EETQ_REQUIRE(x && w && logits_out && top_k_index && top_k_weights, f + ": null pointer");
    const int n_tables = (counts != nullptr) + (offsets != nullptr) + (sorted_slot != nullptr) + (position != nullptr) + (active != nullptr);
    EETQ_REQUIRE(n_tables == 0 || n_tables == 5, f + ": the five table pointers are all null or all set");
    int st = check_select(f, T, E, k, renorm, w_dtype);
    if (st != EETQ_OK) return st;
    EETQ_REQUIRE(H >= 64 && H % 64 == 0, f + ": H must be a multiple of 64");
    EETQ_REQUIRE((long long)T * H < (1ll << 40) && (long long)T * k <= (1ll << 30) && T <= kRouterTokens * 65535,
                 f + ": T * H or T * k too large, or T > 16 * 65535 (one grid row per 16 tokens)");
    EETQ_REQUIRE(aligned16(x) && aligned16(w), f + ": x and w must be 16-byte aligned");
    if (rule) {
        st = check_sigmoid(f, rule->bias, rule->bias_dtype, E, k, rule->n_group, rule->topk_group, rule->scale);
        if (st != EETQ_OK) return st;
    }
    hipStream_t       s   = static_cast<hipStream_t>(stream);
    const int         wpe = waves_per_expert(H), epw = kRouterWaves / wpe, G = (E + epw - 1) / epw;
    const f16*        xp  = static_cast<const f16*>(x);
    const f16*        wp  = static_cast<const f16*>(w);
    const SigmoidRule r   = rule ? *rule : SigmoidRule{};
    const auto        kern = rule ? moe_router_kernel<true> : moe_router_kernel<false>;
    if (T <= kRouterTokens) {
        float*    slab   = nullptr;
        unsigned* ticket = nullptr;
        st = slot_for(s, &slab, &ticket);
        if (st != EETQ_OK) return st;
        static std::atomic<unsigned long long> opted[2];
        st = opt_in_large_lds(kern, opted[rule != nullptr]);
        if (st != EETQ_OK) return st;
        launch_kernel(kern, dim3(G), dim3(kRouterThreads), kLdsFused, s, xp, wp, T, H, E, k, renorm, w_dtype, wpe, logits_out, top_k_index,
                      top_k_weights, counts, offsets, sorted_slot, position, active, slab, ticket, r);
        return check_hip(hipGetLastError(), "moe_router_kernel launch");
    }
    launch_kernel(kern, dim3(G, (T + kRouterTokens - 1) / kRouterTokens), dim3(kRouterThreads), kLdsUsed, s, xp, wp, T, H, E, k, renorm,
                  w_dtype, wpe, logits_out, top_k_index, top_k_weights, static_cast<int*>(nullptr), static_cast<int*>(nullptr),
                  static_cast<int*>(nullptr), static_cast<int*>(nullptr), static_cast<int*>(nullptr), static_cast<float*>(nullptr),
                  static_cast<unsigned*>(nullptr), r);
    st = check_hip(hipGetLastError(), "moe_router_kernel launch");
    if (st != EETQ_OK) return st;
    st = rule ? eetq_moe_topk_sigmoid_f32(logits_out, rule->bias, rule->bias_dtype, T, E, k, rule->n_group, rule->topk_group, renorm,
                                          rule->scale, w_dtype, top_k_index, top_k_weights, stream)
              : eetq_moe_topk_f16(logits_out, T, E, k, renorm, w_dtype, top_k_index, top_k_weights, stream);
    if (st != EETQ_OK || !counts) return st;
    return eetq_moe_route(top_k_index, T, k, E, counts, offsets, sorted_slot, position, active, stream);
}

}  // namespace

int release_moe_router_workspace(size_t* freed)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    int keep = 0;
    (void)hipGetDevice(&keep);
    for (int d = 0; d < 64; ++d) {
        Arena& a = g_arena[d];
        if (a.base && hipSetDevice(d) == hipSuccess) {
            (void)hipDeviceSynchronize();
            (void)hipFree(a.base);
            if (freed) *freed += kArenaBytes;
        }
        a = Arena{};
    }
    (void)hipSetDevice(keep);
    return EETQ_OK;
}

}  // namespace eetq

using namespace eetq;

extern "C" {

int eetq_moe_topk_f16(const void* logits, int T, int E, int k, int renorm, int w_dtype, int64_t* top_k_index, void* top_k_weights,
                      void* stream)
{
    EETQ_REQUIRE(logits && top_k_index && top_k_weights, "eetq_moe_topk_f16: null pointer");
    const int st = check_select("eetq_moe_topk_f16", T, E, k, renorm, w_dtype);
    if (st != EETQ_OK) return st;
    launch_kernel(moe_topk_kernel, dim3((T + kRouterWaves - 1) / kRouterWaves), dim3(kRouterThreads), 0, static_cast<hipStream_t>(stream),
                  static_cast<const f16*>(logits), T, E, k, renorm, w_dtype, top_k_index, top_k_weights);
    return check_hip(hipGetLastError(), "moe_topk_kernel launch");
}

int eetq_moe_topk_sigmoid_f32(const void* logits, const void* bias, int bias_dtype, int T, int E, int k, int n_group, int topk_group,
                              int renorm, float scale, int w_dtype, int64_t* top_k_index, void* top_k_weights, void* stream)
{
    const std::string f = "eetq_moe_topk_sigmoid_f32";
    EETQ_REQUIRE(logits && top_k_index && top_k_weights, f + ": null pointer");
    int st = check_select(f, T, E, k, renorm, w_dtype);
    if (st != EETQ_OK) return st;
    st = check_sigmoid(f, bias, bias_dtype, E, k, n_group, topk_group, scale);
    if (st != EETQ_OK) return st;
    launch_kernel(moe_topk_sigmoid_kernel, dim3((T + kRouterWaves - 1) / kRouterWaves), dim3(kRouterThreads), 0,
                  static_cast<hipStream_t>(stream), static_cast<const float*>(logits), T, E, k, renorm, w_dtype, top_k_index, top_k_weights,
                  SigmoidRule{bias, bias_dtype, n_group, topk_group, scale});
    return check_hip(hipGetLastError(), "moe_topk_sigmoid_kernel launch");
}

int eetq_moe_router_f16(const void* x, const void* w, int T, int H, int E, int k, int renorm, int w_dtype, void* logits_out,
                        int64_t* top_k_index, void* top_k_weights, int* counts, int* offsets, int* sorted_slot, int* position,
                        int* active, void* stream)
{
    return router_entry("eetq_moe_router_f16", x, w, nullptr, T, H, E, k, renorm, w_dtype, logits_out, top_k_index, top_k_weights, counts,
                        offsets, sorted_slot, position, active, stream);
}

int eetq_moe_router_sigmoid_f16(const void* x, const void* w, const void* bias, int bias_dtype, int T, int H, int E, int k, int n_group,
                                int topk_group, int renorm, float scale, int w_dtype, void* logits_out_f32, int64_t* top_k_index,
                                void* top_k_weights, int* counts, int* offsets, int* sorted_slot, int* position, int* active, void* stream)
{
    const SigmoidRule rule{bias, bias_dtype, n_group, topk_group, scale};
    return router_entry("eetq_moe_router_sigmoid_f16", x, w, &rule, T, H, E, k, renorm, w_dtype, logits_out_f32, top_k_index,
                        top_k_weights, counts, offsets, sorted_slot, position, active, stream);
}

}  // extern "C"
