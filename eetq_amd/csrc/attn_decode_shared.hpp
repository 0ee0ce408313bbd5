// The pieces of the decode-attention kernels that do not depend on the cache element: geometry, the lane and workgroup
// merges, the chunk-record merge and its kernel, the in-launch head hand-off, the NeoX rotation of the new token.
// Included by attn_decode.hip (fp16 and int8 rows) and attn_decode_rows.hip; everything is internal to the including file.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace eetq {

namespace {

constexpr int kAttnThreads = 256;
// A chunk record: kRecPad + D floats = [m, l, -, -, o[D]] (o on a 16-byte boundary).
constexpr int kRecPad = 4;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Work assignment (round 6).  The cache rows of a (batch row, kv head) are cut into BLOCKS of BLK = 16 (D = 128) or 32 (D = 64)
// consecutive rows -- one wave-wide 16-byte load per wave covers its share of a block, the workgroup's four waves the whole
// block, 4 or 8 KiB of contiguous bytes -- and chunk `split` of `splits` owns blocks split, split + splits, split + 2 splits, ...:
// all chunks of a head carry the same number of rows to within one block whatever the valid length is.
// A workgroup requests its first kUA + kUB blocks before it consumes anything: at <= (kUA + kUB) * BLK * splits valid rows
// (1536 at 6 chunks, D = 128) every row of the launch is in flight at once and the launch pays the memory latency once
// (rounds 2-5: trips of 4 blocks one ahead -- 5.4 vs 4.7 us for the same bytes as a bare read kernel,
// profiles/r06_attn_probe.txt).  LONG launches (the cache can hold more rows than that) continue in software-pipelined trips
// of kUL blocks.
// Every cache load is an unconditional buffer load, nt (a row is read once per token), through descriptors that END AT THE
// VALID LENGTH: a row that does not count is out of range and comes back as zeros without touching memory -- no load behind a
// branch, no clamped duplicate rows, no select on the way in.  An out-of-range load is not free, though (0.5 us per launch for
// one per block, same probe): the mask loads exist only in the MASK instantiation, the further trips only in the LONG one.
// The running softmax state is rescaled once per trip (A, B, then each further trip), not once per position.
// Measured and shelved (tools/experiments/attn_loader_consumer.patch, profiles/r06_attn_forms.txt): eight waves per workgroup, four
// LOADERS moving the chunk into LDS by LDS-DMA and four consumers taking it from there trip by trip (bit-identical) -- the
// consumers start at 1.6 us instead of 3.4, but the rows arrive later than through registers: 9.9 - 10.7 us per step against 9.4.
constexpr int kUA = 8, kUB = 8, kUL = 4, kUG = 4;
constexpr int kNt = 2;  // aux bits of a buffer load: nt

template <int D>
struct AttnGeo {
    static constexpr int LPP = D / 8;                        // lanes per position
    static constexpr int PPW = 64 / LPP;                     // positions per wave instruction
    static constexpr int BLK = (kAttnThreads / 64) * PPW;    // positions per block
};

// Sum over the LPP = 8 or 16 consecutive lanes that share a position, by DPP (no LDS traffic): quad swaps, then the
// mirrored half row, then the mirrored row.  Every lane of the group ends with the same bits (each step adds the same two
// partial sums in both partners).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
    return v + __builtin_bit_cast(float, moved);
}
template <int LPP>
__device__ __forceinline__ float group_sum(float v)
{
    static_assert(LPP == 8 || LPP == 16, "a position is shared by 8 or 16 lanes");
    v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x141>(v);  // row_half_mirror
    if (LPP == 16) v = dpp_add<0x140>(v);  // row_mirror
    return v;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in order
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

// value of lane ^ OFF (OFF = 8, 16, 32)
template <int OFF>
__device__ __forceinline__ float lane_xor(float v)
{
    const u32 u = __builtin_bit_cast(u32, v);
    if constexpr (OFF == 32) {
        auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        return __builtin_bit_cast(float, (u32)((threadIdx.x & 32) ? r[0] : r[1]));  // r[0]: the lower half everywhere, r[1]: the upper
    } else if constexpr (OFF == 16) {
        auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        return __builtin_bit_cast(float, (u32)((threadIdx.x & 16) ? r[0] : r[1]));  // r[0]: the even 16-lane rows everywhere, r[1]: the odd
    } else {
        return __shfl_xor(v, OFF, 64);
    }
}

// The position groups of a wave (lane swaps, no LDS), then the waves through LDS (NW sets): (m, l, o[8]) per lane -> threads
// tid < D hold (M, L, O) of the chunk.  One barrier; only the consuming waves (kAttnThreads threads) call it.
template <int D>
__device__ __forceinline__ void chunk_merge(float m, float l, const float (&o)[8], float* sm_m, float* sm_l, float* sm_o, float& M,
                                            float& L, float& O)
{
#pragma clang fp contract(off)
    constexpr int LPP = AttnGeo<D>::LPP, PPW = AttnGeo<D>::PPW, NW = kAttnThreads / 64;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane % LPP, d0 = li * 8;
    float mw = m;
    if constexpr (PPW == 8) mw = fmaxf(mw, lane_xor<8>(mw));
    mw = fmaxf(mw, lane_xor<16>(mw));
    mw = fmaxf(mw, lane_xor<32>(mw));
    const float w = mw > -INFINITY ? __expf(m - mw) : 0.f;  // exp(-inf) = 0 for a group without a valid position
    float       part[9];
    part[8] = l * w;
#pragma unroll
    for (int i = 0; i < 8; ++i) part[i] = o[i] * w;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        if constexpr (PPW == 8) part[i] += lane_xor<8>(part[i]);
        part[i] = sum_xor32(sum_xor16(part[i]));
    }
    if (lane < LPP) {
        if (li == 0) {
            sm_m[wave] = mw;
            sm_l[wave] = part[8];
        }
        *reinterpret_cast<f32x4*>(sm_o + wave * D + d0)     = f32x4{part[0], part[1], part[2], part[3]};
        *reinterpret_cast<f32x4*>(sm_o + wave * D + d0 + 4) = f32x4{part[4], part[5], part[6], part[7]};
    }
    __syncthreads();
    M = -INFINITY, L = 0.f, O = 0.f;
    if (tid < D) {
#pragma unroll
        for (int s2 = 0; s2 < NW; ++s2) M = fmaxf(M, sm_m[s2]);
        if (M > -INFINITY) {
#pragma unroll
            for (int s2 = 0; s2 < NW; ++s2) {
                const float ws = __expf(sm_m[s2] - M);  // exp(-inf) = 0 for empty sets
                L = fmaf(sm_l[s2], ws, L);
                O = fmaf(sm_o[s2 * D + tid], ws, O);
            }
        }
    }
}

// rows at and beyond the valid length of a pre-allocated (static) cache hold zeros or stale tokens: never attended
__device__ __forceinline__ int valid_len(int S, const int64_t* kv_len, int kv_len_bias)
{
    return kv_len ? max(0, (int)min((int64_t)S, *kv_len + kv_len_bias)) : S;
}

// how the merge reads records: plain loads in the two-launch form (the records come from an earlier launch), loads served
// below the per-CU L1 in the one-launch form (they come from other workgroups of this launch)
struct PlainRecords {
    const float* base;
    __device__ f32x2 v2(long off) const { return *reinterpret_cast<const f32x2*>(base + off); }
    __device__ f32x4 v4(long off) const { return *reinterpret_cast<const f32x4*>(base + off); }
};
struct CoherentRecords {
    __amdgpu_buffer_rsrc_t rsrc;
    __device__ f32x2 v2(long off) const
    {
        return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)(off * 4), 0, /*sc1*/ 16));
    }
    __device__ f32x4 v4(long off) const
    {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(off * 4), 0, /*sc1*/ 16));
    }
};

// Merge of a head's `splits` chunk records at offsets s * stride (floats) by a workgroup of NT threads (all of them call:
// there is a barrier inside); thread d < D returns channel d, normalised.  The cost of this step is the number of memory
// INSTRUCTIONS a wave issues (~90 cycles each: 51 of them per wave made an earlier form take 3.3 us at 17 records), so:
// lane i of every wave fetches (m, l) of record i with one 8-byte load; a group of D/4 lanes owns a subset of the records
// (every NS-th) and fetches four channels of each with one 16-byte load -- 1 + ceil(splits / NS) loads per wave; the subsets
// are added through lane swaps and one LDS exchange (sm_x: NT/64 * D floats).  Sums run in a fixed order that depends only
// on (D, NT, splits): both launch forms use NT = 256 and give the same bits.  A fully masked row yields zeros, not NaN.
template <int D, int NT, typename Records>
__device__ __forceinline__ float attn_merge(const Records& rec, long stride, int splits, int tid, float* sm_x)
{
#pragma clang fp contract(off)
    constexpr int G = D / 4, WS = 64 / G, NW = NT / 64, NS = NW * WS;  // lanes per record, subsets per wave / per workgroup
    const int lane = tid & 63, wave = tid >> 6, cg = lane % G, rs = wave * WS + lane / G;
    float M = -INFINITY, L = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // one block of up to 64 records, JN loads of this thread's records in flight (JN chosen by the caller from the block's
    // record count: straight-line loads, no load behind a branch)
    auto block = [&](int s0, int n, auto jn_tag) {
        constexpr int JN = decltype(jn_tag)::value;
        f32x4 o4[JN];
#pragma unroll
        for (int j = 0; j < JN; ++j) o4[j] = rec.v4((s0 + min(rs + NS * j, n - 1)) * stride + kRecPad + 4 * cg);
        const f32x2 ml = rec.v2((s0 + min(lane, n - 1)) * stride);
        const float mi = lane < n ? ml.x : -INFINITY, li = lane < n ? ml.y : 0.f;
        float Mb = mi;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) Mb = fmaxf(Mb, __shfl_xor(Mb, off, 64));
        Mb = fmaxf(Mb, M);
        if (Mb > -INFINITY) {  // uniform
            const float keep = __expf(M - Mb);   // 0 for the first block
            const float wi   = __expf(mi - Mb);  // weight of record s0 + lane (exp(-inf) = 0 beyond the block and for empty chunks)
            float x = li * wi;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
            L = fmaf(L, keep, x);
            acc *= keep;
#pragma unroll
            for (int j = 0; j < JN; ++j) {
                const int   idx = rs + NS * j;
                const float w   = __shfl(wi, idx < n ? idx : 0, 64);
                if (idx < n) {
                    acc.x = fmaf(o4[j].x, w, acc.x);
                    acc.y = fmaf(o4[j].y, w, acc.y);
                    acc.z = fmaf(o4[j].z, w, acc.z);
                    acc.w = fmaf(o4[j].w, w, acc.w);
                }
            }
            M = Mb;
        }
    };
    for (int s0 = 0; s0 < splits; s0 += 64) {
        const int n = min(64, splits - s0);
        if (n <= NS)
            block(s0, n, std::integral_constant<int, 1>{});
        else if (n <= 2 * NS)
            block(s0, n, std::integral_constant<int, 2>{});
        else if (n <= 3 * NS)
            block(s0, n, std::integral_constant<int, 3>{});
        else if (n <= 4 * NS)
            block(s0, n, std::integral_constant<int, 4>{});
        else
            block(s0, n, std::integral_constant<int, (64 + NS - 1) / NS>{});
    }
    // the wave's subsets (lanes G apart), then the waves (in order) through LDS
    float part[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (WS == 4) part[c] = sum_xor16(part[c]);
        part[c] = sum_xor32(part[c]);
    }
    if (lane < G) *reinterpret_cast<f32x4*>(sm_x + wave * D + 4 * cg) = f32x4{part[0], part[1], part[2], part[3]};
    __syncthreads();
    if (tid >= D) return 0.f;
    float O = sm_x[tid];
#pragma unroll
    for (int w = 1; w < NW; ++w) O += sm_x[w * D + tid];
    return L > 0.f ? O / L : 0.f;
}

// one workgroup per (head, batch): thread t < splits fetches that chunk's (m, l) in parallel; D threads then sum the chunk
// outputs with the loads of up to 8 chunks in flight
template <int D>
__global__ __launch_bounds__(kAttnThreads) void attn_decode_merge_kernel(const float* __restrict__ ws, f16* __restrict__ out,
                                                                        int splits, long o_sb, long o_sh, int64_t* advance)
{
    __shared__ __attribute__((aligned(16))) float sm_x[(kAttnThreads / 64) * D];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    // workspace [batch][split][head][record]: the records of one head are a row of heads apart
    const PlainRecords rec{ws + ((size_t)b * splits * gridDim.x + h) * (D + kRecPad)};
    const float        o = attn_merge<D, kAttnThreads>(rec, (long)gridDim.x * (D + kRecPad), splits, tid, sm_x);
    if (tid < D) out[b * o_sb + h * o_sh + tid] = (f16)o;
    // the cache's token counter (every reader of it in this step -- the cache-write launch and the partial kernel -- has
    // completed: they are earlier launches on the stream)
    if (advance && h == 0 && b == 0 && tid == 0) *advance += 1;
}

struct RopeAttnArgs {
    const f16 *    q, *k, *v;  // the new token: [batch][heads][D] with q_sb / k_sb / v_sb elements between batch rows
    int            S, groups, kv_len_bias, slot_stride;
    long           kc_sb, kc_sh, kc_ss, vc_sb, vc_sh, vc_ss;
    long           q_sb, k_sb, v_sb;
    const f16*     cos_sin;
    const f16*     mask;
    long           m_sb;
    f16*           out;
    long           o_sb, o_sh;
    float*         ws;
    unsigned*      tickets;  // [batch * heads] per-head arrival counts + [1] finished heads; zero between launches
    int64_t*       advance;
    float          scaling;
    unsigned long long* stamps;  // diagnostics (eetq_diag_attn_stamps): [workgroup][8] device-clock stamps, or null
};

// The per-row first key (PAD instantiations): cache rows below kv_start[b] of batch row b are padding.  Behind the
// plain form's arguments, which keep their kernarg block; the two-launch kernel takes the pointer (or nothing) as its last argument.
struct RopeAttnPadArgs : RopeAttnArgs {
    const int64_t* kv_start;  // DEVICE [batch]
};
template <bool PAD>
using RopeAttnKernArgs = std::conditional_t<PAD, RopeAttnPadArgs, RopeAttnArgs>;
struct NoKvStart {};
template <bool PAD>
using KvStartArg = std::conditional_t<PAD, const int64_t*, NoKvStart>;

// The sliding window (WIN instantiations, built on the PAD arithmetic): batch row b attends the last `window` of its
// n valid rows, i.e. the padded form with kv_start'[b] = max(kv_start[b], n - window); kv_start may be null (then 0).  Behind the
// padded form's arguments; the two-launch kernel takes the pair as its last argument.
struct RopeAttnWinArgs : RopeAttnPadArgs {
    int window;  // >= 1, a host constant of the model
};
struct KvWindow {
    const int64_t* kv_start;  // DEVICE [batch] or null
    int            window;
};
template <bool PAD, bool WIN>
using KvFirstArg = std::conditional_t<WIN, KvWindow, KvStartArg<PAD>>;
// the first row a WIN instantiation hands to clamp_kv_start: the later of the row's own start and the window's first row
__device__ __forceinline__ int64_t window_start(int64_t start, int n, int window) { return max(start, (int64_t)n - (int64_t)window); }

// The first attended row of a batch row: its start, kept inside [0, last] where `last` is the new token's row (one-launch form) or
// the last valid row (two-launch form, no new token) -- a start beyond it attends that row alone, and nothing leaves the cache.
__device__ __forceinline__ int clamp_kv_start(int64_t start, int last)
{
    return (int)max((int64_t)0, min(start, (int64_t)max(last, 0)));
}

// device clock (100 MHz) into slot i of this workgroup's stamp row, ordered behind everything issued so far
#define ATTN_STAMP(i)                                                                                                  \
    do {                                                                                                               \
        if (a.stamps) {                                                                                                \
            unsigned long long t_;                                                                                     \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
            if (threadIdx.x == 0)                                                                                      \
                a.stamps[((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + (i)] = t_;     \
        }                                                                                                              \
    } while (0)


// NeoX rotation of this lane's 8 channels [d0, d0 + 8) of one head (rot_dim = D: channel d < D/2 pairs with d + D/2).
// own / other: the lane's channels and the paired ones; c / s: the lane's 8 values of the position's cos | sin row.  fp16 arithmetic, one rounding per
// multiply and add, exactly rotary_neox_kvcache_kernel (norm_rope.hip).
template <int D>
__device__ __forceinline__ f16x8 rope8(const f16x8& own, const f16x8& other, const f16x8& c, const f16x8& s, int d0)
{
#pragma clang fp contract(off)
    constexpr int embed = D / 2;
    const bool    low   = d0 < embed;
    f16x8         r;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f16 vx = low ? own[i] : other[i], vy = low ? other[i] : own[i];
        const f16 xc = vx * c[i], ys = vy * s[i], yc = vy * c[i], xs = vx * s[i];
        const f16 lo = xc - ys, hi = yc + xs;
        r[i] = low ? lo : hi;
    }
    return r;
}

__device__ __forceinline__ float load_sc1(const float* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // served below the per-CU L1
}
__device__ __forceinline__ void store_sc1(float* p, float v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // write-through
}

// Publish the chunk record, take the head's ticket; the last arriver merges the head's chunks and stores the output, and the last
// head advances the cache's token counter.  Threads tid < D hold the chunk's (M, L, O); kAttnThreads threads call (barriers inside).
template <int D>
__device__ __forceinline__ void head_handoff(const RopeAttnArgs& a, int split, int splits, int h, int b, int H, float M, float L,
                                             float O, float* sm_o, unsigned* sm_ticket)
{
    const int tid = threadIdx.x;
    float*     head_ws = a.ws + ((size_t)b * splits * H + h) * (D + kRecPad);  // [batch][split][head][record]
    const long rec_stride = (long)H * (D + kRecPad);
    if (splits > 1) {
        // ---- publish the chunk record (write-through), take a ticket; every storing wave drains its own stores ----
        if (tid < D) {
            float* rec = head_ws + (size_t)split * rec_stride;
            store_sc1(rec + kRecPad + tid, O);
            if (tid == 0) {
                store_sc1(rec, M);
                store_sc1(rec + 1, L);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        ATTN_STAMP(4);
        if (tid == 0)
            *sm_ticket = __hip_atomic_fetch_add(a.tickets + b * H + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        ATTN_STAMP(5);
        if (*sm_ticket != (unsigned)(splits - 1)) return;  // not the head's last chunk
        if (tid == 0) __hip_atomic_store(a.tickets + b * H + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // ---- last arriver: merge all chunk records of the head (its own one read back like the others) ----
        const CoherentRecords recs{__builtin_amdgcn_make_buffer_rsrc(head_ws, 0, 0x7fffffff, 0x00020000)};
        O = attn_merge<D, kAttnThreads>(recs, rec_stride, splits, tid, sm_o);  // sm_o is free again: reused for the exchange
    } else if (tid < D) {
        O = L > 0.f ? O / L : 0.f;
    }
    ATTN_STAMP(6);
    if (tid < D) a.out[b * a.o_sb + h * a.o_sh + tid] = (f16)O;
    ATTN_STAMP(7);
    // ---- the last head to finish advances the token counter: by then every workgroup of the launch has read it ----
    if (a.advance && tid == 0) {
        const unsigned heads_total = (unsigned)(H * gridDim.z);
        unsigned*      done = a.tickets + heads_total;
        if (__hip_atomic_fetch_add(done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == heads_total - 1) {
            __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *a.advance += 1;
        }
    }
}

// LONG: some chunk may own more than kUA + kUB blocks (a launch-time fact of the capacity S and the chunk count)
template <int D>
bool long_chunks(int S, int splits)
{
    constexpr int BLK = AttnGeo<D>::BLK;
    return ((S + BLK - 1) / BLK + splits - 1) / splits > kUA + kUB;
}

}  // namespace

}  // namespace eetq
