// Single-query ("decode") attention over a KV cache, fp16 in / fp16 out, fp32 softmax and accumulation.
//
// No counterpart in the reference's csrc: its EETLlamaAttention delegates the attention product to flash-attn
// (python/eetq/modules/llama_modules.py:131-143).  The stock library kernel this box offers for a single query token runs
// one workgroup per head (40 workgroups streaming a 25 MB cache: 68 us per layer at Llama-13B shapes), so the decode step
// of eet_accelerator's attention block uses this split-KV form instead: HBM/L2-bound byte work, no MFMA.
//
// Two-launch form (eetq_decode_attention_f16):
//   phase 1  grid (splits, heads, batch), 256 threads: a workgroup owns every splits-th 16-row block of the VALID cache
//            positions (round 6: "Work assignment" below) and has all of them in flight before it consumes any; a group of
//            D/8 lanes owns one position at a time (16-byte loads of its k and v rows, fully coalesced across the wave),
//            keeps an online-softmax state (m, l) and 8 output channels per lane; the groups of a wave are merged by lane
//            swaps, the waves through LDS, and the chunk's (m, l, o[D]) goes to an fp32 workspace;
//   phase 2  grid (heads, batch), 256 threads: merges the chunks (attn_merge), normalises, writes fp16.
// One-launch form (eetq_rope_decode_attention_f16), the decode step of a static cache: the same phase 1 with the NeoX
// rotation of the new token's q and k done in registers on the way in (the arithmetic of rotary_neox_kvcache_kernel, fp16
// with a rounding after every multiply and add), the rotated k and the v written to their cache row by one workgroup per
// kv head, every workgroup taking the new row from registers rather than from the cache (so nothing in the launch reads
// what the launch writes), and phase 2 done by whichever workgroup of a head finishes last: partials are published with
// write-through stores, a ticket per head decides "last" (the in-launch hand-off of gemm_splitk_kernel.hpp), and the last
// head to finish advances the cache's token counter.  Three launches (15.0 us per layer at 13B shapes, 1 k rows) became one
// (10.9 - 11.6 us, rounds 2-5; 9.5 us with the round-6 chunk code, of which 8.7 are there with an almost empty cache: launch
// gap 1.1, scalar reads 0.35, new token + rotation 0.8, the chunk's arithmetic 1.5, workgroup merge 0.4, publish 0.5, ticket
// 0.75, head merge 1.6, store 0.2 -- profiles/r06_attn_stamps.txt, r06_attn_bench.jsonl).  Both forms run the same chunk code
// and the same merge arithmetic: their outputs are bit-identical.
// Both forms also exist with a per-row first key (PAD; eetq_*_padded_f16): batch row b of a left-padded batch
// attends rows [kv_start[b], valid length), its blocks and chunks counted from there.  The plain instantiations are unchanged.
#include "attn_decode_shared.hpp"

namespace eetq {
// decode steps whose new token was NOT written because its cache row was outside the cache (full static cache, negative
// position): stock StaticLayer.update raises there, these kernels skip the write -- and count it here
__device__ unsigned g_attn_dropped = 0;
}  // namespace eetq

namespace eetq {

namespace {

struct KvSrc {
    __amdgpu_buffer_rsrc_t k, v, m;   // the valid rows of one (batch row, kv head); m: the additive mask row (MASK only)
    unsigned               k_row, v_row;  // bytes between cache rows
    unsigned               d0b;           // this lane's channel offset in bytes
};

template <int U>
struct KvBlocks {
    f16x8          k[U], v[U];
    unsigned short m[U];
};

// blocks blk0 + u * dblk for u in [U0, U0 + UN) of the U a KvBlocks holds: this lane's row of each, K and V of a block back
// to back (returns are in order: a block is complete when its V row is)
template <int D, int U0, int UN, bool MASK, int U>
__device__ __forceinline__ void load_range(KvBlocks<U>& t, const KvSrc& s, int blk0, int dblk, int rib)
{
    constexpr int BLK = AttnGeo<D>::BLK;
    static_assert(U0 + UN <= U, "range");
#pragma unroll
    for (int u = U0; u < U0 + UN; ++u) {
        const unsigned j = (unsigned)((blk0 + u * dblk) * BLK + rib);
        t.k[u] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(s.k, (int)(j * s.k_row + s.d0b), 0, kNt));
        t.v[u] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(s.v, (int)(j * s.v_row + s.d0b), 0, kNt));
        if constexpr (MASK) t.m[u] = __builtin_amdgcn_raw_buffer_load_b16(s.m, (int)(j * 2u), 0, 0);
    }
}
template <int D, int U, bool MASK>
__device__ __forceinline__ void load_blocks(KvBlocks<U>& t, const KvSrc& s, int blk0, int dblk, int rib)
{
    load_range<D, 0, U, MASK>(t, s, blk0, dblk, rib);
}

// One trip: the online-softmax update of this lane's running state (m, l, o[8]) with positions [U0, U0 + UN) of the U it holds.
// scores are scaling * (q . k) (+ mask) with the products summed in fp32 (v_dot2_f32_f16); rows >= Sv count for nothing (they
// were out of range of the descriptors: k = v = 0).  SUBST: position `slot` is taken from registers (knew, vnew: this lane's 8
// channels of the new token) instead of the cache -- tested per block (workgroup-uniform), selected per lane inside it.
template <int D, int U0, int UN, bool SUBST, bool MASK, int U>
__device__ __forceinline__ void consume_range(KvBlocks<U>& t, int blk0, int dblk, int rib, int Sv, int slot, const f16x8& knew,
                                              const f16x8& vnew, const f16x2 (&q2)[4], float scaling, float& m, float& l,
                                              float (&o)[8])
{
    // every multiply-add below is explicit and contraction is off: the two launch forms instantiate this code separately
    // and must round identically
#pragma clang fp contract(off)
    static_assert(U0 + UN <= U, "range");
    constexpr int LPP = AttnGeo<D>::LPP, BLK = AttnGeo<D>::BLK;
    if ((blk0 + U0 * dblk) * BLK >= Sv) return;  // workgroup-uniform: the trip's first block is beyond the valid rows, so are the others
    const int     slot_blk = SUBST && slot >= 0 ? slot / BLK : -1;
    float         sc[U];
#pragma unroll
    for (int u = U0; u < U0 + UN; ++u) {
        const int blk = blk0 + u * dblk, j = blk * BLK + rib;
        if (SUBST && blk == slot_blk) {  // workgroup-uniform
            const bool mine = j == slot;
            t.k[u] = mine ? knew : t.k[u];
            t.v[u] = mine ? vnew : t.v[u];
        }
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) a = __builtin_amdgcn_fdot2(f16x2{t.k[u][2 * i], t.k[u][2 * i + 1]}, q2[i], a, false);
        a = group_sum<LPP>(a) * scaling;
        if constexpr (MASK) a += (float)__builtin_bit_cast(f16, t.m[u]);
        sc[u] = j < Sv ? a : -INFINITY;
    }
    float mn = m;
#pragma unroll
    for (int u = U0; u < U0 + UN; ++u) mn = fmaxf(mn, sc[u]);
    if (mn > -INFINITY) {  // group-uniform
        const float keep = __expf(m - mn);
        l *= keep;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] *= keep;
#pragma unroll
        for (int u = U0; u < U0 + UN; ++u) {
            const float p = __expf(sc[u] - mn);  // exp(-inf) = 0 for the positions that do not count
            l += p;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = fmaf(p, (float)t.v[u][i], o[i]);
        }
        m = mn;
    }
}

// The consumption of chunk `split` of one (batch row, head) and its merge across the workgroup.  ta: the chunk's first kUA
// blocks, already requested (load_blocks at blk0 = split, stride splits); tb: registers for the next kUB.  On return
// threads tid < D hold (M, L, O) = the chunk's running maximum, its sum of exp(s - M) and channel tid of sum exp(s - M) v.
// qv: this lane's 8 channels of the (rotated) query.
template <int D, bool SUBST, bool MASK, bool LONG>
__device__ __forceinline__ void attn_chunk(const f16x8& qv, float scaling, KvBlocks<kUA>& ta, KvBlocks<kUB>& tb, const KvSrc& src,
                                           int split, int splits, int Sv, int slot, const f16x8& knew, const f16x8& vnew,
                                           float* sm_m, float* sm_l, float* sm_o, float& M, float& L, float& O)
{
#pragma clang fp contract(off)
    constexpr int LPP = AttnGeo<D>::LPP, PPW = AttnGeo<D>::PPW, BLK = AttnGeo<D>::BLK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int grp = lane / LPP, rib = wave * PPW + grp;
    const f16x2 q2[4] = {{qv[0], qv[1]}, {qv[2], qv[3]}, {qv[4], qv[5]}, {qv[6], qv[7]}};

    float m = -INFINITY, l = 0.f, o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = 0.f;

    // A is on its way (requested by the caller); B is requested here, kUG blocks at a time, between the trips of A: a wave that
    // asks for more than the memory system takes at once is held AT THE REQUEST until there is room, and a wave held there
    // consumes nothing -- with all of B requested up front the first trip of A was consumed 4.2 us into the launch although its
    // rows had landed well before (profiles/r06_attn_stamps.txt).  Trips are kUG blocks each.
    static_assert(kUA == kUB && kUA % kUG == 0, "trip structure");
    const int blk_b = split + kUA * splits;
    auto trips_ab = [&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value;
        load_range<D, I * kUG, kUG, MASK>(tb, src, blk_b, splits, rib);
        __builtin_amdgcn_sched_barrier(0);
        consume_range<D, I * kUG, kUG, SUBST, MASK>(ta, split, splits, rib, Sv, slot, knew, vnew, q2, scaling, m, l, o);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto trips_b = [&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value;
        consume_range<D, I * kUG, kUG, SUBST, MASK>(tb, blk_b, splits, rib, Sv, slot, knew, vnew, q2, scaling, m, l, o);
    };
    constexpr int NT = kUA / kUG;  // trips per batch
    static_for<NT>(trips_ab);
    if constexpr (LONG) {
        // further trips of kUL blocks, software-pipelined one ahead; the first is requested before B is consumed
        const int     nblk = (Sv + BLK - 1) / BLK;
        int           ub   = kUA + kUB;
        KvBlocks<kUL> tl, tn;
        load_blocks<D, kUL, MASK>(tl, src, split + ub * splits, splits, rib);
        __builtin_amdgcn_sched_barrier(0);
        static_for<NT>(trips_b);
        while (split + ub * splits < nblk) {  // workgroup-uniform
            load_blocks<D, kUL, MASK>(tn, src, split + (ub + kUL) * splits, splits, rib);
            consume_range<D, 0, kUL, SUBST, MASK>(tl, split + ub * splits, splits, rib, Sv, slot, knew, vnew, q2, scaling, m, l, o);
            tl = tn;
            ub += kUL;
        }
    } else {
        static_for<NT>(trips_b);
    }

    chunk_merge<D>(m, l, o, sm_m, sm_l, sm_o, M, L, O);
}

// the buffer descriptors of one (batch row, kv head), ending at the valid length Sv
template <int D, bool MASK>
__device__ __forceinline__ KvSrc make_kv_src(const f16* kbase, const f16* vbase, long k_ss, long v_ss, int Sv, const f16* mrow)
{
    KvSrc s;
    s.k_row = (unsigned)(k_ss * 2);
    s.v_row = (unsigned)(v_ss * 2);
    s.d0b   = (unsigned)(((threadIdx.x & 63) % AttnGeo<D>::LPP) * 16);
    s.k = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(kbase), 0, (int)((unsigned)Sv * s.k_row), 0x00020000);
    s.v = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(vbase), 0, (int)((unsigned)Sv * s.v_row), 0x00020000);
    s.m = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(MASK ? mrow : kbase), 0, MASK ? Sv * 2 : 0, 0x00020000);
    return s;
}

// PAD: batch row b attends rows [s, Sv), s = kv_start[b] kept inside the valid rows: the K, V and mask bases move by s rows and the
// valid length is taken relative to s, so blocks and chunks are counted from the row's first real token (the bits of the plain form
// on that row alone, its cache moved up by s rows) and no row below s is read.
template <int D, bool MASK, bool LONG, bool PAD = false>
__global__ __launch_bounds__(kAttnThreads) void attn_decode_partial_kernel(
    const f16* __restrict__ q, const f16* __restrict__ kc, const f16* __restrict__ vc, const f16* __restrict__ mask,
    float* __restrict__ ws, float scaling, int S, int groups, long q_sb, long q_sh, long k_sb, long k_sh,
    long k_ss, long v_sb, long v_sh, long v_ss, long m_sb, const int64_t* __restrict__ kv_len, int kv_len_bias,
    const KvStartArg<PAD> kv_start)
{
    constexpr int NW = kAttnThreads / 64;
    __shared__ float sm_m[NW], sm_l[NW];
    __shared__ __attribute__((aligned(16))) float sm_o[NW * D];

    const int split = blockIdx.x, splits = gridDim.x, h = blockIdx.y, b = blockIdx.z, hk = h / groups;
    const int tid = threadIdx.x, d0 = ((tid & 63) % (D / 8)) * 8;
    const int rib = (tid >> 6) * AttnGeo<D>::PPW + (tid & 63) / AttnGeo<D>::LPP;
    int  Sv = valid_len(S, kv_len, kv_len_bias);
    long s0 = 0;  // PAD: the row's first attended cache row
    if constexpr (PAD) {
        s0 = clamp_kv_start(kv_start[b], Sv - 1);
        Sv -= (int)s0;
    }

    const f16x8 qv  = *reinterpret_cast<const f16x8*>(q + b * q_sb + h * q_sh + d0);
    const KvSrc src = make_kv_src<D, MASK>(kc + b * k_sb + hk * k_sh + s0 * k_ss, vc + b * v_sb + hk * v_sh + s0 * v_ss, k_ss, v_ss, Sv,
                                           MASK ? mask + b * m_sb + s0 : nullptr);
    KvBlocks<kUA> ta;
    KvBlocks<kUB> tb;
    load_blocks<D, kUA, MASK>(ta, src, split, splits, rib);
    float       M, L, O;
    const f16x8 none = {};
    attn_chunk<D, false, MASK, LONG>(qv, scaling, ta, tb, src, split, splits, Sv, -1, none, none, sm_m, sm_l, sm_o, M, L, O);
    if (tid < D) {
        float* out = ws + (((size_t)b * gridDim.x + split) * gridDim.y + h) * (D + kRecPad);  // [batch][split][head][record]
        out[kRecPad + tid] = O;
        if (tid == 0) {
            out[0] = M;
            out[1] = L;
        }
    }
}


// grid (splits, heads, batch), 256 threads; see the file header.  The five leading pointers are preloaded into SGPRs at
// launch (-amdgpu-kernarg-preload-count): the three scalar reads the chunk bounds depend on go out with the first
// instructions, together with the fetch of the argument block, and nothing else stands before the first cache loads.
//
// PAD: a fourth scalar read, kv_start[b], joins the batch (one wait, still no branch before the cache loads).  With s the start kept
// inside [0, slot], the K, V and mask bases move by s rows, the valid length and the slot the chunk code sees are taken relative to
// s (as in attn_decode_partial_kernel<.., PAD>: the two forms stay bit-identical); the new row is written at its absolute slot.
template <int D, bool MASK, bool LONG, bool PAD = false>
__global__ __launch_bounds__(kAttnThreads) void rope_attn_decode_kernel(const int64_t* __restrict__ kv_len,
                                                                        const int64_t* __restrict__ slots,
                                                                        const int64_t* __restrict__ positions,
                                                                        f16* __restrict__ kc, f16* __restrict__ vc,
                                                                        const RopeAttnKernArgs<PAD> a)
{
    constexpr int LPP = D / 8, NW = kAttnThreads / 64;
    __shared__ float    sm_m[NW], sm_l[NW];
    __shared__ __attribute__((aligned(16))) float sm_o[NW * D];
    __shared__ unsigned sm_ticket;

    ATTN_STAMP(0);
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z, hk = h / a.groups;
    const int splits = gridDim.x, H = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, li = lane % LPP, d0 = li * 8;
    const int d1 = d0 < D / 2 ? d0 + D / 2 : d0 - D / 2;  // the paired channels of the rotation

    // three independent scalar reads, every one from a valid address (no branch before the loads): a missing `slots`
    // reads the position instead, a missing `kv_len` reads the position and ignores it
    // (issued as one batch with one wait: left to itself the compiler waits after each of them).  They go out with the first
    // instructions, on a quiet memory system (0.3 - 0.6 us): behind a burst of cache loads the same reads take 1.2 us and
    // hold back everything that depends on the valid length (measured: profiles/r06_attn_stamps.txt).
    const int64_t* p_pos  = positions + b;
    const int64_t* p_slot = slots ? slots + (long)b * a.slot_stride : positions + b;
    const int64_t* p_len  = kv_len ? kv_len : positions;
    int64_t        rpos, slot64, filled, start64 = 0;
    if constexpr (PAD) {
        const int64_t* p_start = a.kv_start + b;
        asm volatile("s_load_dwordx2 %0, %4, 0x0\n\ts_load_dwordx2 %1, %5, 0x0\n\ts_load_dwordx2 %2, %6, 0x0\n\t"
                     "s_load_dwordx2 %3, %7, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(rpos), "=&s"(slot64), "=&s"(filled), "=&s"(start64)
                     : "s"(p_pos), "s"(p_slot), "s"(p_len), "s"(p_start)
                     : "memory");
    } else {
        asm volatile("s_load_dwordx2 %0, %3, 0x0\n\ts_load_dwordx2 %1, %4, 0x0\n\ts_load_dwordx2 %2, %5, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(rpos), "=&s"(slot64), "=&s"(filled)
                     : "s"(p_pos), "s"(p_slot), "s"(p_len)
                     : "memory");
    }
    ATTN_STAMP(1);
    // a slot outside the cache is neither written nor attended, and (like the two-launch form) nothing is rotated then
    // (no upper bound on rpos here, unlike the two-launch form: launch_rope_attn_decode's table_rows)
    const bool have_new = slot64 >= 0 && slot64 < a.S && rpos >= 0;
    const int  slot = have_new ? (int)slot64 : -1;
    // a full cache (or a bad position) used to be silent: count the dropped steps (eetq_decode_dropped_steps)
    if (!have_new && split == 0 && h == 0 && threadIdx.x == 0) atomicAdd(&g_attn_dropped, 1u);
    const int  Sv_all = kv_len ? max(0, (int)min((int64_t)a.S, filled + a.kv_len_bias)) : a.S;
    // PAD: everything the chunk code sees is relative to the row's first attended row s0 (scalar arithmetic, no branch)
    const long s0     = PAD ? clamp_kv_start(start64, have_new ? slot : Sv_all - 1) : 0;
    const int  Sv     = PAD ? max(0, Sv_all - (int)s0) : Sv_all;
    const int  slot_c = PAD && have_new ? slot - (int)s0 : slot;

    // Memory queue order (a wave's loads return in order): the new token and its cos | sin row first, then the chunk's first
    // kUA blocks; the rotation runs on the former while the latter are on their way; attn_chunk requests the rest.
    const f16*  qp = a.q + b * a.q_sb + (long)h * D;
    const f16*  kp = a.k + b * a.k_sb + (long)hk * D;
    f16x8       qv   = *reinterpret_cast<const f16x8*>(qp + d0);
    f16x8       knew = *reinterpret_cast<const f16x8*>(kp + d0);
    const f16x8 vnew = *reinterpret_cast<const f16x8*>(a.v + b * a.v_sb + (long)hk * D + d0);
    const f16x8 qpair = *reinterpret_cast<const f16x8*>(qp + d1), kpair = *reinterpret_cast<const f16x8*>(kp + d1);
    // (a bad position reads row 0 of the table and is not used)
    const f16*  cs = a.cos_sin + (have_new ? rpos : 0) * D + (d0 < D / 2 ? d0 : d0 - D / 2);
    const f16x8 rc = *reinterpret_cast<const f16x8*>(cs), rs = *reinterpret_cast<const f16x8*>(cs + D / 2);
    __builtin_amdgcn_sched_barrier(0);  // (the scheduler sinks these seven loads below the block loads otherwise)
    const KvSrc src = make_kv_src<D, MASK>(kc + b * a.kc_sb + hk * a.kc_sh + s0 * a.kc_ss, vc + b * a.vc_sb + hk * a.vc_sh + s0 * a.vc_ss,
                                           a.kc_ss, a.vc_ss, Sv, MASK ? a.mask + b * a.m_sb + s0 : nullptr);
    const int   rib = (tid >> 6) * AttnGeo<D>::PPW + lane / LPP;
    KvBlocks<kUA> ta;
    KvBlocks<kUB> tb;
    load_blocks<D, kUA, MASK>(ta, src, split, splits, rib);
    __builtin_amdgcn_sched_barrier(0);
    if (have_new) {
        qv   = rope8<D>(qv, qpair, rc, rs, d0);
        knew = rope8<D>(knew, kpair, rc, rs, d0);
    }
    __builtin_amdgcn_sched_barrier(0);
    // the cache row of the new token: once per kv head, by one position group of the head's first workgroup
    if (have_new && split == 0 && h == hk * a.groups && tid < LPP) {
        *reinterpret_cast<f16x8*>(kc + b * a.kc_sb + hk * a.kc_sh + (long)slot * a.kc_ss + d0) = knew;
        *reinterpret_cast<f16x8*>(vc + b * a.vc_sb + hk * a.vc_sh + (long)slot * a.vc_ss + d0) = vnew;
    }
    ATTN_STAMP(2);
    float M, L, O;
    attn_chunk<D, true, MASK, LONG>(qv, a.scaling, ta, tb, src, split, splits, Sv, slot_c, knew, vnew, sm_m, sm_l, sm_o, M, L, O);

    ATTN_STAMP(3);
    head_handoff<D>(a, split, splits, h, b, H, M, L, O, sm_o, &sm_ticket);
}


template <int D, bool MASK, bool LONG, bool PAD>
int launch_d2(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv, int S,
              int splits, float scaling, const long* st, const int64_t* kv_len, int kv_len_bias, int64_t* advance,
              hipStream_t stream, KvStartArg<PAD> kv_start)
{
    launch_kernel(attn_decode_partial_kernel<D, MASK, LONG, PAD>, dim3(splits, H, B), dim3(kAttnThreads), 0, stream, q, k, v, mask, ws,
                  scaling, S, H / Hkv, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], kv_len, kv_len_bias, kv_start);
    EETQ_TRY_HIP(hipGetLastError());
    launch_kernel(attn_decode_merge_kernel<D>, dim3(H, B), dim3(kAttnThreads), 0, stream, (const float*)ws, out, splits, st[9],
                  st[10], advance);
    return check_hip(hipGetLastError(), "attn_decode kernels launch");
}

template <int D, bool PAD>
int launch_d(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv, int S,
             int splits, float scaling, const long* st, const int64_t* kv_len, int kv_len_bias, int64_t* advance,
             hipStream_t stream, KvStartArg<PAD> kv_start)
{
    const bool lng = long_chunks<D>(S, splits);
#define EETQ_ATTN_GO(MASK, LONG)                                                                                                  \
    return launch_d2<D, MASK, LONG, PAD>(q, k, v, mask, out, ws, B, H, Hkv, S, splits, scaling, st, kv_len, kv_len_bias, advance, \
                                         stream, kv_start)
    if (mask) {
        if (lng) EETQ_ATTN_GO(true, true);
        EETQ_ATTN_GO(true, false);
    }
    if (lng) EETQ_ATTN_GO(false, true);
    EETQ_ATTN_GO(false, false);
#undef EETQ_ATTN_GO
}

template <int D, bool PAD>
int launch_rope_d(const int64_t* kv_len, const int64_t* slots, const int64_t* positions, f16* kc, f16* vc,
                  const RopeAttnKernArgs<PAD>& a, dim3 grid, hipStream_t stream)
{
    const bool lng = long_chunks<D>(a.S, (int)grid.x);
#define EETQ_ATTN_GO(MASK, LONG) \
    launch_kernel(rope_attn_decode_kernel<D, MASK, LONG, PAD>, grid, dim3(kAttnThreads), 0, stream, kv_len, slots, positions, kc, vc, a)
    if (a.mask) {
        if (lng) EETQ_ATTN_GO(true, true);
        else EETQ_ATTN_GO(true, false);
    } else {
        if (lng) EETQ_ATTN_GO(false, true);
        else EETQ_ATTN_GO(false, false);
    }
#undef EETQ_ATTN_GO
    return check_hip(hipGetLastError(), "rope_attn_decode_kernel launch");
}

}  // namespace

namespace {
template <bool PAD>
int launch_attn_decode_any(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv,
                           int S, int D, int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                           int64_t* advance, hipStream_t stream, KvStartArg<PAD> kv_start)
{
    EETQ_REQUIRE(q && k && v && out && ws && strides, "null pointer");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && S > 0 && splits > 0 && splits <= S, "invalid attention shape");
    for (int i = 0; i < 9; ++i)
        if (i != 8) EETQ_REQUIRE(strides[i] % 8 == 0, "q / k / v strides must be multiples of 8 elements (16-byte loads)");
    EETQ_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0, "q, k, v must be 16-byte aligned");
    EETQ_REQUIRE(strides[4] > 0 && strides[7] > 0 && ((long)S + 4096) * strides[4] * 2 < (1L << 31) &&
                     ((long)S + 4096) * strides[7] * 2 < (1L << 31),
                 "one head's cache rows must span less than 2 GiB");
    if (D == 128)
        return launch_d<128, PAD>(q, k, v, mask, out, ws, B, H, Hkv, S, splits, scaling, strides, kv_len, kv_len_bias, advance, stream,
                                  kv_start);
    if (D == 64)
        return launch_d<64, PAD>(q, k, v, mask, out, ws, B, H, Hkv, S, splits, scaling, strides, kv_len, kv_len_bias, advance, stream,
                                 kv_start);
    return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] decode attention supports head_dim 64 and 128");
}
}  // namespace

int launch_attn_decode(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv,
                       int S, int D, int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                       int64_t* advance, hipStream_t stream)
{
    return launch_attn_decode_any<false>(q, k, v, mask, out, ws, B, H, Hkv, S, D, splits, scaling, strides, kv_len, kv_len_bias,
                                         advance, stream, NoKvStart{});
}

// launch_attn_decode with a per-row first key: batch row b attends cache rows [kv_start[b], valid length) (DEVICE [B])
int launch_attn_decode_padded(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv,
                              int S, int D, int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                              const int64_t* kv_start, int64_t* advance, hipStream_t stream)
{
    EETQ_REQUIRE(kv_start, "null kv_start");
    return launch_attn_decode_any<true>(q, k, v, mask, out, ws, B, H, Hkv, S, D, splits, scaling, strides, kv_len, kv_len_bias,
                                        advance, stream, kv_start);
}

static unsigned long long* g_attn_stamps = nullptr;  // process-wide diagnostic hook (not thread-safe by design)
void set_attn_stamps(unsigned long long* buf) { g_attn_stamps = buf; }

namespace {
template <bool PAD>
int launch_rope_attn_decode_any(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                                const f16* v, const f16* cos_sin, f16* kc, f16* vc, const f16* mask, f16* out, float* ws,
                                unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                                const long* st, const int64_t* kv_len, int kv_len_bias, const int64_t* kv_start, int64_t* advance,
                                long table_rows, hipStream_t stream)
{
    EETQ_REQUIRE(positions && q && k && v && cos_sin && kc && vc && out && ws && tickets && st, "null pointer");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && S > 0 && splits > 0 && splits <= S && splits <= 4096,
                 "invalid attention shape");
    // validated, not yet enforced on the device: with the compare in have_new the attention term of the decode budget measured
    // above the parent's run-to-run spread, so the kernel is as it was
    EETQ_REQUIRE(table_rows > 0, "the cos|sin table must have at least one row");
    for (int i = 0; i < 9; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q / k / v / cache strides must be multiples of 8 elements (16-byte accesses)");
    EETQ_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)cos_sin) % 16 == 0,
                 "q, k, v, the caches and the cos|sin table must be 16-byte aligned");
    EETQ_REQUIRE(st[5] > 0 && st[8] > 0 && ((long)S + 4096) * st[5] * 2 < (1L << 31) && ((long)S + 4096) * st[8] * 2 < (1L << 31),
                 "one head's cache rows must span less than 2 GiB");
    RopeAttnKernArgs<PAD> a;
    if constexpr (PAD) a.kv_start = kv_start;
    a.slot_stride = slot_stride;
    a.q = q, a.k = k, a.v = v, a.q_sb = st[0], a.k_sb = st[1], a.v_sb = st[2];
    a.cos_sin = cos_sin;
    a.kc_sb = st[3], a.kc_sh = st[4], a.kc_ss = st[5], a.vc_sb = st[6], a.vc_sh = st[7], a.vc_ss = st[8];
    a.mask = mask, a.m_sb = st[9], a.out = out, a.o_sb = st[10], a.o_sh = st[11];
    a.ws = ws, a.tickets = tickets, a.kv_len_bias = kv_len_bias, a.advance = advance;
    a.S = S, a.groups = H / Hkv, a.scaling = scaling;
    a.stamps = g_attn_stamps;
    if (D == 128) return launch_rope_d<128, PAD>(kv_len, slots, positions, kc, vc, a, dim3(splits, H, B), stream);
    if (D == 64) return launch_rope_d<64, PAD>(kv_len, slots, positions, kc, vc, a, dim3(splits, H, B), stream);
    return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] decode attention supports head_dim 64 and 128");
}
}  // namespace

int launch_rope_attn_decode(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                            const f16* v, const f16* cos_sin, f16* kc, f16* vc, const f16* mask, f16* out, float* ws,
                            unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                            const long* st, const int64_t* kv_len, int kv_len_bias, int64_t* advance, long table_rows,
                            hipStream_t stream)
{
    return launch_rope_attn_decode_any<false>(positions, slots, slot_stride, q, k, v, cos_sin, kc, vc, mask, out, ws, tickets, B, H,
                                              Hkv, S, D, splits, scaling, st, kv_len, kv_len_bias, nullptr, advance, table_rows,
                                              stream);
}

// launch_rope_attn_decode with a per-row first key: batch row b attends cache rows [kv_start[b], valid length) (DEVICE [B])
int launch_rope_attn_decode_padded(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                                   const f16* v, const f16* cos_sin, f16* kc, f16* vc, const f16* mask, f16* out, float* ws,
                                   unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                                   const long* st, const int64_t* kv_len, int kv_len_bias, const int64_t* kv_start,
                                   int64_t* advance, long table_rows, hipStream_t stream)
{
    EETQ_REQUIRE(kv_start, "null kv_start");
    return launch_rope_attn_decode_any<true>(positions, slots, slot_stride, q, k, v, cos_sin, kc, vc, mask, out, ws, tickets, B, H,
                                             Hkv, S, D, splits, scaling, st, kv_len, kv_len_bias, kv_start, advance, table_rows,
                                             stream);
}

}  // namespace eetq

namespace eetq {
int attn_dropped_steps(unsigned* count, bool reset)
{
    EETQ_TRY_HIP(hipMemcpyFromSymbol(count, HIP_SYMBOL(g_attn_dropped), sizeof(unsigned)));
    if (reset) {
        const unsigned zero = 0;
        EETQ_TRY_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_attn_dropped), &zero, sizeof(unsigned)));
    }
    return EETQ_OK;
}
}  // namespace eetq
