// Single-query ("decode") attention over a KV cache of fp16 rows or of int8 rows (kv_i8.hpp): fp16 in / fp16 out,
// fp32 softmax and accumulation.  One set of kernels over a row-format policy (KvF16, KvI8).
//
// No counterpart in the reference's csrc: its EETLlamaAttention delegates the attention product to flash-attn
// (python/eetq/modules/llama_modules.py:131-143).  The stock library kernel this box offers for a single query token runs
// one workgroup per head (40 workgroups streaming a 25 MB cache: 68 us per layer at Llama-13B shapes), so the decode step
// of eet_accelerator's attention block uses this split-KV form instead: HBM/L2-bound byte work, no MFMA.
//
// Two-launch form (eetq_decode_attention_f16, eetq_decode_attention_i8kv_f16):
//   phase 1  grid (splits, heads, batch), 256 threads: a workgroup owns every splits-th 16-row block of the VALID cache
//            positions (round 6: "Work assignment" in attn_decode_shared.hpp) and has all of them in flight before it consumes
//            any; a group of D/8 lanes owns one position at a time (16-byte loads of its k and v rows, fully coalesced across
//            the wave), keeps an online-softmax state (m, l) and 8 output channels per lane; the groups of a wave are merged by
//            lane swaps, the waves through LDS, and the chunk's (m, l, o[D]) goes to an fp32 workspace;
//   phase 2  grid (heads, batch), 256 threads: merges the chunks (attn_merge), normalises, writes fp16.
// One-launch form (eetq_rope_decode_attention_f16, eetq_rope_decode_attention_i8kv_f16), the decode step of a static cache: the
// same phase 1 with the NeoX rotation of the new token's q and k done in registers on the way in (the arithmetic of
// rotary_neox_kvcache_kernel, fp16 with a rounding after every multiply and add), the rotated k and the v written to their
// cache row by one workgroup per kv head, every workgroup taking the new row from registers rather than from the cache (so
// nothing in the launch reads what the launch writes), and phase 2 done by whichever workgroup of a head finishes last:
// partials are published with write-through stores, a ticket per head decides "last" (the in-launch hand-off of
// gemm_splitk_kernel.hpp), and the last head to finish advances the cache's token counter.  Three launches (15.0 us per layer
// at 13B shapes, 1 k rows) became one (10.9 - 11.6 us, rounds 2-5; 9.5 us with the round-6 chunk code, of which 8.7 are there
// with an almost empty cache: launch gap 1.1, scalar reads 0.35, new token + rotation 0.8, the chunk's arithmetic 1.5,
// workgroup merge 0.4, publish 0.5, ticket 0.75, head merge 1.6, store 0.2 -- profiles/r06_attn_stamps.txt,
// r06_attn_bench.jsonl).  Both forms run the same chunk code and the same merge arithmetic: their outputs are bit-identical.
// The fp16 forms also exist with a per-row first key (PAD; eetq_*_padded_f16): batch row b of a left-padded
// batch attends rows [kv_start[b], valid length), its blocks and chunks counted from there.  The plain instantiations are
// unchanged.  On top of PAD, a sliding window (WIN; eetq_*_window_f16): the first row becomes
// max(kv_start[b], valid length - window), one scalar maximum in front of the padded form's arithmetic.  On top of WIN, a ring
// cache (RING; eetq_*_ring_f16): the same rows counted from the same first row, addressed modulo the cache's rows.
//
// What the cache element changes is held by the row-format policy and nothing else does:
//   KvF16  a lane's share of a row is 16 bytes of K and 16 of V, used as loaded;
//   KvI8   8 bytes of each, and the row's scale pair comes with one dword load through a third descriptor that ends at the
//          valid length as well: a row that does not count returns bytes 0, scale 0.  Bytes become fp16 pairs by the
//          biased-byte trick (exact integers), q . k8 is summed in fp32 by v_dot2_f32_f16 and the K scale is folded into the
//          score (ks * scaling) * (q . k8), the V scale into the probability: o += (p * vs) * v8; vs * v8 is exact in fp32, so a
//          row that holds all the weight comes out as fp16(vs * v8) bit for bit.  The one-launch form quantises the new
//          token's rotated K and its V in registers, writes bytes and scale pair from one position group per kv head, and
//          every workgroup attends the new row as its quantised self from registers.
// The loaders and the two online-softmax bodies (load_range, consume_range) stay whole, one overload per format: sharing their skeleton over small per-format
// helpers reorders the fp16 kernels' instructions (docs/HISTORY.md, "Decode attention: one kernel template").
#include "attn_decode_shared.hpp"
#include "kv_i8.hpp"

namespace eetq {
// decode steps whose new token was NOT written because its cache row was outside the cache (full static cache, negative
// position): stock StaticLayer.update raises there, these kernels skip the write -- and count it here (both row formats)
__device__ unsigned g_attn_dropped = 0;
}  // namespace eetq

namespace eetq {

namespace {

// ---- fp16 rows ----
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
// the new token's row: this lane's 8 channels, as loaded (k rotated)
struct NewRow16 {
    f16x8 k, v;
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

// One trip: the online-softmax update of this lane's running state (m, l, o[8]) with positions [U0, U0 + UN) of the U it holds.
// scores are scaling * (q . k) (+ mask) with the products summed in fp32 (v_dot2_f32_f16); rows >= Sv count for nothing (they
// were out of range of the descriptors: k = v = 0).  SUBST: position `slot` is taken from registers (nw: this lane's 8
// channels of the new token) instead of the cache -- tested per block (workgroup-uniform), selected per lane inside it.
template <int D, int U0, int UN, bool SUBST, bool MASK, int U>
__device__ __forceinline__ void consume_range(KvBlocks<U>& t, int blk0, int dblk, int rib, int Sv, int slot, const NewRow16& nw,
                                              const f16x2 (&q2)[4], float scaling, float& m, float& l, float (&o)[8])
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
            t.k[u] = mine ? nw.k : t.k[u];
            t.v[u] = mine ? nw.v : t.v[u];
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

struct KvF16 {
    using Elem = f16;
    struct Scales {};  // none
    template <bool PAD, bool WIN = false>
    using RopeArgs = std::conditional_t<WIN, RopeAttnWinArgs, RopeAttnKernArgs<PAD>>;
    template <typename A>
    static __device__ __forceinline__ Scales scales(const A&) { return {}; }
    static __device__ __forceinline__ Scales rows(const Scales&, int, int) { return {}; }
    static constexpr bool kStamps = true;  // the one-launch kernel carries the device-clock stamps (eetq_diag_attn_stamps)

    using Src = KvSrc;
    template <int U>
    using Blocks = KvBlocks<U>;
    using New = NewRow16;

    // the loader and the consumer of this format, as attn_chunk calls them.  One forwarding level on purpose: with the bodies as
    // members, or with attn_chunk calling the overloads itself, the compiler inlines in another order and every kernel comes out
    // as the same instructions in another order (docs/HISTORY.md, "Decode attention: one kernel template")
    template <int D, int U0, int UN, bool MASK, int U>
    static __device__ __forceinline__ void load(Blocks<U>& t, const Src& s, int blk0, int dblk, int rib)
    {
        load_range<D, U0, UN, MASK>(t, s, blk0, dblk, rib);
    }
    template <int D, int U0, int UN, bool SUBST, bool MASK, int U>
    static __device__ __forceinline__ void consume(Blocks<U>& t, int blk0, int dblk, int rib, int Sv, int slot, const New& nw,
                                                   const f16x2 (&q2)[4], float scaling, float& m, float& l, float (&o)[8])
    {
        consume_range<D, U0, UN, SUBST, MASK>(t, blk0, dblk, rib, Sv, slot, nw, q2, scaling, m, l, o);
    }

    // the buffer descriptors of one (batch row, kv head), ending at the valid length Sv; strides in fp16 elements
    template <int D, bool MASK>
    static __device__ __forceinline__ Src make_src(const f16* kbase, const f16* vbase, const Scales&, long k_ss, long v_ss, int Sv,
                                                   const f16* mrow)
    {
        Src s;
        s.k_row = (unsigned)(k_ss * 2);
        s.v_row = (unsigned)(v_ss * 2);
        s.d0b   = (unsigned)(((threadIdx.x & 63) % AttnGeo<D>::LPP) * 16);
        s.k = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(kbase), 0, (int)((unsigned)Sv * s.k_row), 0x00020000);
        s.v = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(vbase), 0, (int)((unsigned)Sv * s.v_row), 0x00020000);
        s.m = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(MASK ? mrow : kbase), 0, MASK ? Sv * 2 : 0, 0x00020000);
        return s;
    }

    template <int LPP>
    static __device__ __forceinline__ void make_new(New& nw, const f16x8& knew, const f16x8& vnew)
    {
        nw.k = knew;
        nw.v = vnew;
    }
    // the new token's cache row of (batch row b, kv head hk): called by one position group (tid < LPP)
    static __device__ __forceinline__ void store_new(const RopeAttnArgs& a, f16* kc, f16* vc, int b, int hk, int slot, const New& nw,
                                                     int d0)
    {
        *reinterpret_cast<f16x8*>(kc + b * a.kc_sb + hk * a.kc_sh + (long)slot * a.kc_ss + d0) = nw.k;
        *reinterpret_cast<f16x8*>(vc + b * a.vc_sb + hk * a.vc_sh + (long)slot * a.vc_ss + d0) = nw.v;
    }

    // ---- host: what the entries refuse and say ----
    static constexpr const char* kBadHeadDim   = "[eetq_amd] decode attention supports head_dim 64 and 128";
    static constexpr const char* kTwoLaunch    = "attn_decode kernels launch";
    static constexpr const char* kOneLaunch    = "rope_attn_decode_kernel launch";
    static constexpr bool        kSlotStride01 = false;  // the fp16 one-launch entry takes any slot_stride (as it always has)
    static int check_rows(int S, long k_ss, long v_ss)
    {
        EETQ_REQUIRE(k_ss > 0 && v_ss > 0 && ((long)S + 4096) * k_ss * 2 < (1L << 31) && ((long)S + 4096) * v_ss * 2 < (1L << 31),
                     "one head's cache rows must span less than 2 GiB");
        return EETQ_OK;
    }
    // st: q_b, q_h, then the six cache strides, mask, out (launch_attn_decode)
    static int check_two_launch(const f16* q, const f16* k, const f16* v, const Scales&, int S, const long* st)
    {
        for (int i = 0; i < 8; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q / k / v strides must be multiples of 8 elements (16-byte loads)");
        EETQ_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0, "q, k, v must be 16-byte aligned");
        return check_rows(S, st[4], st[7]);
    }
    // st: q_b, k_b, v_b, then the six cache strides (launch_rope_attn_decode)
    static int check_one_launch(const f16* q, const f16* k, const f16* v, const f16* cos_sin, const f16* kc, const f16* vc,
                                const Scales&, int S, const long* st)
    {
        for (int i = 0; i < 9; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q / k / v / cache strides must be multiples of 8 elements (16-byte accesses)");
        EETQ_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)cos_sin) % 16 == 0,
                     "q, k, v, the caches and the cos|sin table must be 16-byte aligned");
        return check_rows(S, st[5], st[8]);
    }
};

// ---- fp16 rows of a ring cache (RING) ----
// Logical row r of the sequence lives at physical row r mod R.  The chunk code keeps counting rows from the first attended row s0;
// only the address changes: the descriptors cover the R rows of the ring from physical row 0, relative row i is physical row
// p0 + i (p0 = s0 mod R), less R where that passes the end -- one compare-subtract per lane, no division --, and rows i >= Sv, which
// the descriptors of the static forms clip, are sent out of range here (they read as zeros there and here).
struct KvSrcRing : KvSrc {
    unsigned p0, rows, valid;  // s0 mod R; R; Sv
};
constexpr unsigned kRingOob = 0x7ffffff0u;  // beyond any descriptor (check_rows: one head's rows span less than 2 GiB - 4096 rows)

template <int D, int U0, int UN, int U>
__device__ __forceinline__ void load_range_ring(KvBlocks<U>& t, const KvSrcRing& s, int blk0, int dblk, int rib)
{
    constexpr int BLK = AttnGeo<D>::BLK;
    static_assert(U0 + UN <= U, "range");
#pragma unroll
    for (int u = U0; u < U0 + UN; ++u) {
        const unsigned i  = (unsigned)((blk0 + u * dblk) * BLK + rib);
        const unsigned p  = s.p0 + i;
        const unsigned j  = p >= s.rows ? p - s.rows : p;
        const bool     in = i < s.valid;
        t.k[u] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(s.k, (int)(in ? j * s.k_row + s.d0b : kRingOob), 0, kNt));
        t.v[u] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(s.v, (int)(in ? j * s.v_row + s.d0b : kRingOob), 0, kNt));
    }
}

struct KvF16Ring : KvF16 {
    using Src = KvSrcRing;
    template <int D, int U0, int UN, bool MASK, int U>
    static __device__ __forceinline__ void load(Blocks<U>& t, const Src& s, int blk0, int dblk, int rib)
    {
        static_assert(!MASK, "no additive mask on a ring");
        load_range_ring<D, U0, UN>(t, s, blk0, dblk, rib);
    }
    // the descriptors of one (batch row, kv head): all R rows from physical row 0; s0: the first attended logical row, Sv: the rows
    // attended from there (kept <= R: more cannot be live)
    template <int D>
    static __device__ __forceinline__ Src make_ring_src(const f16* kbase, const f16* vbase, long k_ss, long v_ss, int R, int s0, int Sv)
    {
        Src s;
        s.k_row = (unsigned)(k_ss * 2);
        s.v_row = (unsigned)(v_ss * 2);
        s.d0b   = (unsigned)(((threadIdx.x & 63) % AttnGeo<D>::LPP) * 16);
        s.k = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(kbase), 0, (int)((unsigned)R * s.k_row), 0x00020000);
        s.v = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(vbase), 0, (int)((unsigned)R * s.v_row), 0x00020000);
        s.m = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(kbase), 0, 0, 0x00020000);
        s.p0    = (unsigned)s0 % (unsigned)R;
        s.rows  = (unsigned)R;
        s.valid = (unsigned)Sv;
        return s;
    }
};

// ---- int8 rows, one dword of scales per row (kv_i8.hpp) ----
struct ScaleStrides {
    long sb, sh, ss;  // fp16 elements between batch rows, kv heads, rows of the scale tensor
};

// max over the LPP lanes that share a position: group_sum's DPP ladder with max
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v)
{
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
    return fmaxf(v, __builtin_bit_cast(float, moved));
}
template <int LPP>
__device__ __forceinline__ float group_max(float v)
{
    static_assert(LPP == 8 || LPP == 16, "a position is shared by 8 or 16 lanes");
    v = dpp_max<0xB1>(v);
    v = dpp_max<0x4E>(v);
    v = dpp_max<0x141>(v);
    if (LPP == 16) v = dpp_max<0x140>(v);
    return v;
}

struct KvSrc8 {
    __amdgpu_buffer_rsrc_t k, v, m, s;  // the valid rows of one (batch row, kv head); s: their scale pairs; m: the mask row (MASK only)
    unsigned               k_row, v_row, s_row;  // bytes between cache rows / scale pairs
    unsigned               d0b;                  // this lane's channel offset in bytes
};
template <int U>
struct KvBlocks8 {
    u32x2          k[U], v[U];
    u32            s[U];  // (k scale, v scale) as two fp16
    unsigned short m[U];
};
// the new token's row as the cache will hold it
struct NewRow8 {
    u32x2 k, v;  // this lane's 8 bytes
    u32   s;     // the row's scale pair
};

template <int D, int U0, int UN, bool MASK, int U>
__device__ __forceinline__ void load_range(KvBlocks8<U>& t, const KvSrc8& s, int blk0, int dblk, int rib)
{
    constexpr int BLK = AttnGeo<D>::BLK;
    static_assert(U0 + UN <= U, "range");
#pragma unroll
    for (int u = U0; u < U0 + UN; ++u) {
        const unsigned j = (unsigned)((blk0 + u * dblk) * BLK + rib);
        t.k[u] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(s.k, (int)(j * s.k_row + s.d0b), 0, kNt));
        t.v[u] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(s.v, (int)(j * s.v_row + s.d0b), 0, kNt));
        t.s[u] = __builtin_amdgcn_raw_buffer_load_b32(s.s, (int)(j * s.s_row), 0, kNt);
        if constexpr (MASK) t.m[u] = __builtin_amdgcn_raw_buffer_load_b16(s.m, (int)(j * 2u), 0, 0);
    }
}

// consume_range on int8 rows
template <int D, int U0, int UN, bool SUBST, bool MASK, int U>
__device__ __forceinline__ void consume_range(KvBlocks8<U>& t, int blk0, int dblk, int rib, int Sv, int slot, const NewRow8& nw,
                                              const f16x2 (&q2)[4], float scaling, float& m, float& l, float (&o)[8])
{
#pragma clang fp contract(off)
    static_assert(U0 + UN <= U, "range");
    constexpr int LPP = AttnGeo<D>::LPP, BLK = AttnGeo<D>::BLK;
    if ((blk0 + U0 * dblk) * BLK >= Sv) return;  // workgroup-uniform
    const int slot_blk = SUBST && slot >= 0 ? slot / BLK : -1;
    float     sc[U];
#pragma unroll
    for (int u = U0; u < U0 + UN; ++u) {
        const int blk = blk0 + u * dblk, j = blk * BLK + rib;
        if (SUBST && blk == slot_blk) {  // workgroup-uniform
            const bool mine = j == slot;
            t.k[u] = mine ? nw.k : t.k[u];
            t.v[u] = mine ? nw.v : t.v[u];
            t.s[u] = mine ? nw.s : t.s[u];
        }
        f16x2 kh[4];
        kv8_unpack8(t.k[u], kh);
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) a = __builtin_amdgcn_fdot2(kh[i], q2[i], a, false);
        a = group_sum<LPP>(a) * ((float)as_f16x2(t.s[u])[0] * scaling);
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
            const float p = __expf(sc[u] - mn);
            l += p;
            const float pv = p * (float)as_f16x2(t.s[u])[1];
            f16x2       vh[4];
            kv8_unpack8(t.v[u], vh);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = fmaf(pv, (float)vh[i >> 1][i & 1], o[i]);
        }
        m = mn;
    }
}

struct KvI8 {
    using Elem = int8_t;
    struct Scales {
        f16*         p;  // [.., 2]: (k scale, v scale) of every row
        ScaleStrides st;
    };
    struct RopeArgs8 : RopeAttnArgs {  // kc_* / vc_* strides in bytes
        Scales sc;
    };
    template <bool PAD, bool WIN = false>
    using RopeArgs = RopeArgs8;  // (no per-row first key and no window on int8 rows)
    static __device__ __forceinline__ const Scales& scales(const RopeArgs8& a) { return a.sc; }
    // the scale pairs of one (batch row, kv head)
    static __device__ __forceinline__ Scales rows(const Scales& sc, int b, int hk) { return {sc.p + b * sc.st.sb + hk * sc.st.sh, sc.st}; }
    static constexpr bool kStamps = false;

    using Src = KvSrc8;
    template <int U>
    using Blocks = KvBlocks8<U>;
    using New = NewRow8;

    // (one forwarding level, as in KvF16)
    template <int D, int U0, int UN, bool MASK, int U>
    static __device__ __forceinline__ void load(Blocks<U>& t, const Src& s, int blk0, int dblk, int rib)
    {
        load_range<D, U0, UN, MASK>(t, s, blk0, dblk, rib);
    }
    template <int D, int U0, int UN, bool SUBST, bool MASK, int U>
    static __device__ __forceinline__ void consume(Blocks<U>& t, int blk0, int dblk, int rib, int Sv, int slot, const New& nw,
                                                   const f16x2 (&q2)[4], float scaling, float& m, float& l, float (&o)[8])
    {
        consume_range<D, U0, UN, SUBST, MASK>(t, blk0, dblk, rib, Sv, slot, nw, q2, scaling, m, l, o);
    }

    // the buffer descriptors of one (batch row, kv head), all three ending at the valid length Sv; strides in bytes (k, v) and
    // fp16 elements (scales)
    template <int D, bool MASK>
    static __device__ __forceinline__ Src make_src(const int8_t* kbase, const int8_t* vbase, const Scales& rows, long k_ss, long v_ss,
                                                   int Sv, const f16* mrow)
    {
        const f16* sbase = rows.p;
        Src        s;
        s.k_row = (unsigned)k_ss;
        s.v_row = (unsigned)v_ss;
        s.s_row = (unsigned)(rows.st.ss * 2);
        s.d0b   = (unsigned)(((threadIdx.x & 63) % AttnGeo<D>::LPP) * 8);
        s.k = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(kbase), 0, (int)((unsigned)Sv * s.k_row), 0x00020000);
        s.v = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(vbase), 0, (int)((unsigned)Sv * s.v_row), 0x00020000);
        s.s = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(sbase), 0, (int)((unsigned)Sv * s.s_row), 0x00020000);
        s.m = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(MASK ? mrow : sbase), 0, MASK ? Sv * 2 : 0, 0x00020000);
        return s;
    }

    // the row as the cache holds it: every position group of every workgroup has the whole row across its LPP lanes
    template <int LPP>
    static __device__ __forceinline__ void make_new(New& nw, const f16x8& knew, const f16x8& vnew)
    {
        const f16 ks = kv8_scale(group_max<LPP>(kv8_abs_max8(knew))), vs = kv8_scale(group_max<LPP>(kv8_abs_max8(vnew)));
        nw.k = kv8_quant8(knew, ks);
        nw.v = kv8_quant8(vnew, vs);
        nw.s = as_u32(f16x2{ks, vs});
        __builtin_amdgcn_sched_barrier(0);
    }
    static __device__ __forceinline__ void store_new(const RopeArgs8& a, int8_t* kc, int8_t* vc, int b, int hk, int slot,
                                                     const New& nw, int d0)
    {
        *reinterpret_cast<u32x2*>(kc + b * a.kc_sb + hk * a.kc_sh + (long)slot * a.kc_ss + d0) = nw.k;
        *reinterpret_cast<u32x2*>(vc + b * a.vc_sb + hk * a.vc_sh + (long)slot * a.vc_ss + d0) = nw.v;
        if (threadIdx.x == 0) *reinterpret_cast<u32*>(a.sc.p + b * a.sc.st.sb + hk * a.sc.st.sh + (long)slot * a.sc.st.ss) = nw.s;
    }

    // ---- host ----
    static constexpr const char* kBadHeadDim   = "[eetq_amd] decode attention on an int8 cache supports head_dim 64 and 128";
    static constexpr const char* kTwoLaunch    = "attn_decode_i8 kernels launch";
    static constexpr const char* kOneLaunch    = "rope_attn_decode_i8_kernel launch";
    static constexpr bool        kSlotStride01 = true;
    static int check_cache(const int8_t* k, const int8_t* v, const Scales& sc, int S, const long* cst)
    {
        const long sst[3] = {sc.st.sb, sc.st.sh, sc.st.ss};
        return check_i8_cache(k, v, sc.p, S, cst, sst);
    }
    static int check_two_launch(const f16* q, const int8_t* k, const int8_t* v, const Scales& sc, int S, const long* st)
    {
        EETQ_REQUIRE(st[0] % 8 == 0 && st[1] % 8 == 0, "q strides must be multiples of 8 elements (16-byte loads)");
        EETQ_REQUIRE((uintptr_t)q % 16 == 0, "q must be 16-byte aligned");
        return check_cache(k, v, sc, S, st + 2);
    }
    static int check_one_launch(const f16* q, const f16* k, const f16* v, const f16* cos_sin, const int8_t* kc, const int8_t* vc,
                                const Scales& sc, int S, const long* st)
    {
        for (int i = 0; i < 3; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q / k / v strides must be multiples of 8 elements (16-byte accesses)");
        EETQ_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)cos_sin) % 16 == 0,
                     "q, k, v and the cos|sin table must be 16-byte aligned");
        return check_cache(kc, vc, sc, S, st + 3);
    }
};

// The consumption of chunk `split` of one (batch row, head) and its merge across the workgroup.  ta: the chunk's first kUA
// blocks, already requested (Row::load at blk0 = split, stride splits); tb: registers for the next kUB.  On return
// threads tid < D hold (M, L, O) = the chunk's running maximum, its sum of exp(s - M) and channel tid of sum exp(s - M) v.
// qv: this lane's 8 channels of the (rotated) query.
template <class Row, int D, bool SUBST, bool MASK, bool LONG>
__device__ __forceinline__ void attn_chunk(const f16x8& qv, float scaling, typename Row::template Blocks<kUA>& ta,
                                           typename Row::template Blocks<kUB>& tb, const typename Row::Src& src, int split,
                                           int splits, int Sv, int slot, const typename Row::New& nw, float* sm_m, float* sm_l,
                                           float* sm_o, float& M, float& L, float& O)
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
        Row::template load<D, I * kUG, kUG, MASK>(tb, src, blk_b, splits, rib);
        __builtin_amdgcn_sched_barrier(0);
        Row::template consume<D, I * kUG, kUG, SUBST, MASK>(ta, split, splits, rib, Sv, slot, nw, q2, scaling, m, l, o);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto trips_b = [&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value;
        Row::template consume<D, I * kUG, kUG, SUBST, MASK>(tb, blk_b, splits, rib, Sv, slot, nw, q2, scaling, m, l, o);
    };
    constexpr int NT = kUA / kUG;  // trips per batch
    static_for<NT>(trips_ab);
    if constexpr (LONG) {
        // further trips of kUL blocks, software-pipelined one ahead; the first is requested before B is consumed
        const int                           nblk = (Sv + BLK - 1) / BLK;
        int                                 ub   = kUA + kUB;
        typename Row::template Blocks<kUL> tl, tn;
        Row::template load<D, 0, kUL, MASK>(tl, src, split + ub * splits, splits, rib);
        __builtin_amdgcn_sched_barrier(0);
        static_for<NT>(trips_b);
        while (split + ub * splits < nblk) {  // workgroup-uniform
            Row::template load<D, 0, kUL, MASK>(tn, src, split + (ub + kUL) * splits, splits, rib);
            Row::template consume<D, 0, kUL, SUBST, MASK>(tl, split + ub * splits, splits, rib, Sv, slot, nw, q2, scaling, m, l, o);
            tl = tn;
            ub += kUL;
        }
    } else {
        static_for<NT>(trips_b);
    }

    chunk_merge<D>(m, l, o, sm_m, sm_l, sm_o, M, L, O);
}

// Phase 1 of the two-launch form: one chunk of one (batch row, head) into its record of the workspace.
// PAD: batch row b attends rows [s, Sv), s = kv_start[b] kept inside the valid rows: the K, V and mask bases move by s rows and the
// valid length is taken relative to s, so blocks and chunks are counted from the row's first real token (the bits of the plain form
// on that row alone, its cache moved up by s rows) and no row below s is read.
// WIN (with PAD): s = max(kv_start[b] or 0, valid length - window) first, then the same: the bits of the PAD form given that start.
// RING (with WIN, no kv_start, no mask): S is the ring's row count R and the valid length is logical (it may exceed R); the first
// row s0 = max(0, n - window) and the rows counted from it are those of the WIN form, their addresses wrap (KvF16Ring).
template <class Row, int D, bool MASK, bool LONG, bool PAD, bool WIN = false, bool RING = false>
__device__ __forceinline__ void attn_partial(const f16* __restrict__ q, const typename Row::Elem* __restrict__ kc,
                                             const typename Row::Elem* __restrict__ vc, const typename Row::Scales& sc,
                                             const f16* __restrict__ mask, float* __restrict__ ws, float scaling, int S, int groups,
                                             long q_sb, long q_sh, long k_sb, long k_sh, long k_ss, long v_sb, long v_sh, long v_ss,
                                             long m_sb, const int64_t* __restrict__ kv_len, int kv_len_bias,
                                             const KvFirstArg<PAD, WIN> kv_start)
{
    static_assert(!WIN || PAD, "the window is built on the per-row first key");
    static_assert(!RING || (WIN && !MASK), "the ring is built on the window, without a mask");
    constexpr int NW = kAttnThreads / 64;
    __shared__ float sm_m[NW], sm_l[NW];
    __shared__ __attribute__((aligned(16))) float sm_o[NW * D];

    const int split = blockIdx.x, splits = gridDim.x, h = blockIdx.y, b = blockIdx.z, hk = h / groups;
    const int tid = threadIdx.x, d0 = ((tid & 63) % (D / 8)) * 8;
    const int rib = (tid >> 6) * AttnGeo<D>::PPW + (tid & 63) / AttnGeo<D>::LPP;
    int  Sv = valid_len(RING ? INT32_MAX : S, kv_len, kv_len_bias);
    long s0 = 0;  // PAD: the row's first attended cache row
    if constexpr (RING) {
        s0 = clamp_kv_start(window_start(0, Sv, kv_start.window), Sv - 1);
        Sv = min(Sv - (int)s0, S);
    } else if constexpr (WIN) {
        // a missing kv_start reads a valid address instead and counts as 0 (selects, no branch before the loads)
        const int64_t* p_start = kv_start.kv_start ? kv_start.kv_start + b : reinterpret_cast<const int64_t*>(q);
        const int64_t  start   = kv_start.kv_start ? *p_start : 0;
        s0 = clamp_kv_start(window_start(start, Sv, kv_start.window), Sv - 1);
        Sv -= (int)s0;
    } else if constexpr (PAD) {
        s0 = clamp_kv_start(kv_start[b], Sv - 1);
        Sv -= (int)s0;
    }

    const f16x8 qv = *reinterpret_cast<const f16x8*>(q + b * q_sb + h * q_sh + d0);
    const typename Row::Src src = [&] {
        if constexpr (RING)
            return Row::template make_ring_src<D>(kc + b * k_sb + hk * k_sh, vc + b * v_sb + hk * v_sh, k_ss, v_ss, S, (int)s0, Sv);
        else
            return Row::template make_src<D, MASK>(kc + b * k_sb + hk * k_sh + s0 * k_ss, vc + b * v_sb + hk * v_sh + s0 * v_ss,
                                                   Row::rows(sc, b, hk), k_ss, v_ss, Sv, MASK ? mask + b * m_sb + s0 : nullptr);
    }();
    typename Row::template Blocks<kUA> ta;
    typename Row::template Blocks<kUB> tb;
    Row::template load<D, 0, kUA, MASK>(ta, src, split, splits, rib);
    float                    M, L, O;
    const typename Row::New none = {};
    attn_chunk<Row, D, false, MASK, LONG>(qv, scaling, ta, tb, src, split, splits, Sv, -1, none, sm_m, sm_l, sm_o, M, L, O);
    if (tid < D) {
        float* out = ws + (((size_t)b * gridDim.x + split) * gridDim.y + h) * (D + kRecPad);  // [batch][split][head][record]
        out[kRecPad + tid] = O;
        if (tid == 0) {
            out[0] = M;
            out[1] = L;
        }
    }
}

// its two argument lists (the int8 one carries the scale tensor and its strides)
template <int D, bool MASK, bool LONG, bool PAD = false, bool WIN = false, bool RING = false>
__global__ __launch_bounds__(kAttnThreads) void attn_decode_partial_kernel(
    const f16* __restrict__ q, const f16* __restrict__ kc, const f16* __restrict__ vc, const f16* __restrict__ mask,
    float* __restrict__ ws, float scaling, int S, int groups, long q_sb, long q_sh, long k_sb, long k_sh,
    long k_ss, long v_sb, long v_sh, long v_ss, long m_sb, const int64_t* __restrict__ kv_len, int kv_len_bias,
    const KvFirstArg<PAD, WIN> kv_start)
{
    attn_partial<std::conditional_t<RING, KvF16Ring, KvF16>, D, MASK, LONG, PAD, WIN, RING>(
        q, kc, vc, KvF16::Scales{}, mask, ws, scaling, S, groups, q_sb, q_sh, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss, m_sb, kv_len, kv_len_bias,
        kv_start);
}
template <int D, bool MASK, bool LONG>
__global__ __launch_bounds__(kAttnThreads) void attn_decode_partial_i8_kernel(
    const f16* __restrict__ q, const int8_t* __restrict__ kc, const int8_t* __restrict__ vc, const f16* __restrict__ scales,
    const f16* __restrict__ mask, float* __restrict__ ws, float scaling, int S, int groups, long q_sb, long q_sh, long k_sb,
    long k_sh, long k_ss, long v_sb, long v_sh, long v_ss, long m_sb, ScaleStrides sst, const int64_t* __restrict__ kv_len,
    int kv_len_bias)
{
    attn_partial<KvI8, D, MASK, LONG, false>(q, kc, vc, KvI8::Scales{const_cast<f16*>(scales), sst}, mask, ws, scaling, S, groups, q_sb,
                                             q_sh, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss, m_sb, kv_len, kv_len_bias, NoKvStart{});
}

#define ATTN_ROW_STAMP(i) \
    if constexpr (Row::kStamps) ATTN_STAMP(i)

// grid (splits, heads, batch), 256 threads; see the file header.  The five leading pointers are preloaded into SGPRs at
// launch (-amdgpu-kernarg-preload-count): the three scalar reads the chunk bounds depend on go out with the first
// instructions, together with the fetch of the argument block, and nothing else stands before the first cache loads.
//
// PAD: a fourth scalar read, kv_start[b], joins the batch (one wait, still no branch before the cache loads).  With s the start kept
// inside [0, slot], the K, V and mask bases move by s rows, the valid length and the slot the chunk code sees are taken relative to
// s (as in attn_partial<.., PAD>: the two forms stay bit-identical); the new row is written at its absolute slot.
//
// WIN (with PAD): the same four reads -- a missing kv_start reads the position instead and counts as 0 --, then s = max(s, n - window)
// with n = slot + 1 (the new token counts; without a new token the valid length), scalar arithmetic, and the PAD code as it is.
//
// RING (Row = KvF16Ring, with WIN, no kv_start, no mask; kv_len given): a.S is the ring's row count R.  The new token's logical slot
// is its position in the sequence, so `have_new` has no upper bound -- a ring is never full; a bad position still drops the step and
// counts --, the valid length is logical, and s, the rows counted from it and the slot the chunk code sees are the WIN form's.  The
// bases stay at physical row 0, the loads wrap (KvF16Ring) and the new row is written at slot mod R = (s mod R) + (slot - s), less R
// where that passes the end.  The fourth scalar read is the position again, unused: the batch and its one wait are the WIN form's.
template <class Row, int D, bool MASK, bool LONG, bool PAD = false, bool WIN = false, bool RING = false>
__global__ __launch_bounds__(kAttnThreads) void rope_attn_decode_kernel(const int64_t* __restrict__ kv_len,
                                                                        const int64_t* __restrict__ slots,
                                                                        const int64_t* __restrict__ positions,
                                                                        typename Row::Elem* __restrict__ kc,
                                                                        typename Row::Elem* __restrict__ vc,
                                                                        const typename Row::template RopeArgs<PAD, WIN> a)
{
    static_assert(!WIN || PAD, "the window is built on the per-row first key");
    static_assert(!RING || (WIN && !MASK), "the ring is built on the window, without a mask");
    constexpr int LPP = D / 8, NW = kAttnThreads / 64;
    __shared__ float    sm_m[NW], sm_l[NW];
    __shared__ __attribute__((aligned(16))) float sm_o[NW * D];
    __shared__ unsigned sm_ticket;

    ATTN_ROW_STAMP(0);
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
        const int64_t* p_start = WIN && !a.kv_start ? positions + b : a.kv_start + b;
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
    ATTN_ROW_STAMP(1);
    // a slot outside the cache is neither written nor attended, and (like the two-launch form) nothing is rotated then
    // (no upper bound on rpos here, unlike the two-launch form: launch_rope_attn's table_rows)
    const bool have_new = slot64 >= 0 && slot64 < (RING ? (int64_t)INT32_MAX : (int64_t)a.S) && rpos >= 0;
    const int  slot = have_new ? (int)slot64 : -1;
    // a full cache (or a bad position) used to be silent: count the dropped steps (eetq_decode_dropped_steps)
    if (!have_new && split == 0 && h == 0 && threadIdx.x == 0) atomicAdd(&g_attn_dropped, 1u);
    const int  Sv_all = kv_len ? max(0, (int)min((int64_t)(RING ? INT32_MAX : a.S), filled + a.kv_len_bias)) : a.S;
    if constexpr (WIN) start64 = window_start(a.kv_start ? start64 : 0, have_new ? slot + 1 : Sv_all, a.window);
    // PAD: everything the chunk code sees is relative to the row's first attended row s0 (scalar arithmetic, no branch)
    const long s0     = PAD ? clamp_kv_start(start64, have_new ? slot : Sv_all - 1) : 0;
    const int  Sv     = RING ? min(max(0, Sv_all - (int)s0), a.S) : PAD ? max(0, Sv_all - (int)s0) : Sv_all;
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
    const typename Row::Src src = [&] {
        if constexpr (RING)
            return Row::template make_ring_src<D>(kc + b * a.kc_sb + hk * a.kc_sh, vc + b * a.vc_sb + hk * a.vc_sh, a.kc_ss, a.vc_ss, a.S,
                                                  (int)s0, Sv);
        else
            return Row::template make_src<D, MASK>(kc + b * a.kc_sb + hk * a.kc_sh + s0 * a.kc_ss,
                                                   vc + b * a.vc_sb + hk * a.vc_sh + s0 * a.vc_ss, Row::rows(Row::scales(a), b, hk),
                                                   a.kc_ss, a.vc_ss, Sv, MASK ? a.mask + b * a.m_sb + s0 : nullptr);
    }();
    const int   rib = (tid >> 6) * AttnGeo<D>::PPW + lane / LPP;
    typename Row::template Blocks<kUA> ta;
    typename Row::template Blocks<kUB> tb;
    Row::template load<D, 0, kUA, MASK>(ta, src, split, splits, rib);
    __builtin_amdgcn_sched_barrier(0);
    if (have_new) {
        qv   = rope8<D>(qv, qpair, rc, rs, d0);
        knew = rope8<D>(knew, kpair, rc, rs, d0);
    }
    __builtin_amdgcn_sched_barrier(0);
    typename Row::New nw;
    Row::template make_new<LPP>(nw, knew, vnew);
    // the cache row of the new token: once per kv head, by one position group of the head's first workgroup
    int wslot = slot;  // RING: the physical row of the new token
    if constexpr (RING) {
        const unsigned p = src.p0 + (unsigned)slot_c;
        wslot = (int)(p >= src.rows ? p - src.rows : p);
    }
    if (have_new && split == 0 && h == hk * a.groups && tid < LPP) Row::store_new(a, kc, vc, b, hk, wslot, nw, d0);
    ATTN_ROW_STAMP(2);
    float M, L, O;
    attn_chunk<Row, D, true, MASK, LONG>(qv, a.scaling, ta, tb, src, split, splits, Sv, slot_c, nw, sm_m, sm_l, sm_o, M, L, O);

    ATTN_ROW_STAMP(3);
    head_handoff<D>(a, split, splits, h, b, H, M, L, O, sm_o, &sm_ticket);
}

// what the decode entries of a ring cache refuse (S: the ring's rows R)
inline int check_ring(int R, int window, const int64_t* kv_start, const f16* mask, const int64_t* kv_len)
{
    EETQ_REQUIRE(window >= 1, "the attention window must be at least 1 row");
    EETQ_REQUIRE(R >= window, "a ring cache must have at least `window` rows (the live rows of a decode step)");
    EETQ_REQUIRE(!kv_start, "ring and kv_start exclude each other (no ragged ring)");
    EETQ_REQUIRE(!mask, "ring and an additive mask exclude each other (the mask row would need the same wrap)");
    EETQ_REQUIRE(kv_len, "a ring cache needs the device length kv_len (its valid length is logical, not the capacity)");
    return EETQ_OK;
}

// f(D, MASK, LONG as integral constants) for the launch's head_dim, mask and capacity: the instantiation ladder
template <typename F>
int dispatch_attn(int D, bool mask, int S, int splits, const char* bad_head_dim, F f)
{
    auto go = [&](auto d) {
        const bool lng = long_chunks<decltype(d)::value>(S, splits);
        if (mask) return lng ? f(d, std::true_type{}, std::true_type{}) : f(d, std::true_type{}, std::false_type{});
        return lng ? f(d, std::false_type{}, std::true_type{}) : f(d, std::false_type{}, std::false_type{});
    };
    if (D == 128) return go(std::integral_constant<int, 128>{});
    if (D == 64) return go(std::integral_constant<int, 64>{});
    return fail(EETQ_ERR_UNSUPPORTED, bad_head_dim);
}

template <int D, bool MASK, bool LONG, bool PAD, bool WIN, bool RING>
void launch_partial(dim3 grid, hipStream_t stream, const f16* q, const f16* k, const f16* v, const KvF16::Scales&, const f16* mask,
                    float* ws, float scaling, int S, int groups, const long* st, const int64_t* kv_len, int kv_len_bias,
                    KvFirstArg<PAD, WIN> kv_start)
{
    launch_kernel(attn_decode_partial_kernel<D, MASK, LONG, PAD, WIN, RING && !MASK>, grid, dim3(kAttnThreads), 0, stream, q, k, v, mask, ws, scaling, S,
                  groups, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], kv_len, kv_len_bias, kv_start);
}
template <int D, bool MASK, bool LONG, bool PAD, bool WIN, bool RING>
void launch_partial(dim3 grid, hipStream_t stream, const f16* q, const int8_t* k, const int8_t* v, const KvI8::Scales& sc,
                    const f16* mask, float* ws, float scaling, int S, int groups, const long* st, const int64_t* kv_len,
                    int kv_len_bias, NoKvStart)
{
    launch_kernel(attn_decode_partial_i8_kernel<D, MASK, LONG>, grid, dim3(kAttnThreads), 0, stream, q, k, v, (const f16*)sc.p, mask, ws,
                  scaling, S, groups, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], sc.st, kv_len, kv_len_bias);
}

// the two-launch form over either row format; strides: q_b, q_h, the cache's six, mask_b, out_b, out_h
template <class Row, bool PAD, bool WIN = false, bool RING = false>
int launch_attn(const f16* q, const typename Row::Elem* k, const typename Row::Elem* v, const typename Row::Scales& sc, const f16* mask,
                f16* out, float* ws, int B, int H, int Hkv, int S, int D, int splits, float scaling, const long* st,
                const int64_t* kv_len, int kv_len_bias, int64_t* advance, hipStream_t stream, KvFirstArg<PAD, WIN> kv_start)
{
    EETQ_REQUIRE(q && k && v && out && ws && st, "null pointer");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && S > 0 && splits > 0 && splits <= S, "invalid attention shape");
    if constexpr (RING) {
        const int rc = check_ring(S, kv_start.window, kv_start.kv_start, mask, kv_len);
        if (rc != EETQ_OK) return rc;
    }
    const int rc = Row::check_two_launch(q, k, v, sc, S, st);
    if (rc != EETQ_OK) return rc;
    return dispatch_attn(D, mask != nullptr, S, splits, Row::kBadHeadDim, [&](auto d, auto m, auto l) {
        constexpr int DD = decltype(d)::value;
        launch_partial<DD, decltype(m)::value, decltype(l)::value, PAD, WIN, RING>(dim3(splits, H, B), stream, q, k, v, sc, mask, ws, scaling, S,
                                                                        H / Hkv, st, kv_len, kv_len_bias, kv_start);
        EETQ_TRY_HIP(hipGetLastError());
        launch_kernel(attn_decode_merge_kernel<DD>, dim3(H, B), dim3(kAttnThreads), 0, stream, (const float*)ws, out, splits, st[9],
                      st[10], advance);
        return check_hip(hipGetLastError(), Row::kTwoLaunch);
    });
}

unsigned long long* g_attn_stamps = nullptr;  // process-wide diagnostic hook (not thread-safe by design)

// the one-launch form over either row format; st: q_b, k_b, v_b, the cache's six, mask_b, out_b, out_h
template <class Row, bool PAD, bool WIN = false, bool RING = false>
int launch_rope_attn(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k, const f16* v,
                     const f16* cos_sin, typename Row::Elem* kc, typename Row::Elem* vc, const typename Row::Scales& sc,
                     const f16* mask, f16* out, float* ws, unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits,
                     float scaling, const long* st, const int64_t* kv_len, int kv_len_bias, const int64_t* kv_start,
                     int64_t* advance, long table_rows, hipStream_t stream, int window = 0)
{
    EETQ_REQUIRE(positions && q && k && v && cos_sin && kc && vc && out && ws && tickets && st, "null pointer");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && S > 0 && splits > 0 && splits <= S && splits <= 4096,
                 "invalid attention shape");
    if (Row::kSlotStride01) EETQ_REQUIRE(slot_stride == 0 || slot_stride == 1, "slot_stride must be 0 (one slot for the batch) or 1");
    // validated, not yet enforced on the device: with the compare in have_new the attention term of the decode budget measured
    // above the parent's run-to-run spread, so the kernel is as it was
    EETQ_REQUIRE(table_rows > 0, "the cos|sin table must have at least one row");
    if constexpr (RING) {
        const int rc = check_ring(S, window, kv_start, mask, kv_len);
        if (rc != EETQ_OK) return rc;
    }
    const int rc = Row::check_one_launch(q, k, v, cos_sin, kc, vc, sc, S, st);
    if (rc != EETQ_OK) return rc;
    typename Row::template RopeArgs<PAD, WIN> a;
    if constexpr (PAD) a.kv_start = kv_start;
    if constexpr (WIN) a.window = window;
    if constexpr (!std::is_empty_v<typename Row::Scales>) a.sc = sc;
    a.slot_stride = slot_stride;
    a.q = q, a.k = k, a.v = v, a.q_sb = st[0], a.k_sb = st[1], a.v_sb = st[2];
    a.cos_sin = cos_sin;
    a.kc_sb = st[3], a.kc_sh = st[4], a.kc_ss = st[5], a.vc_sb = st[6], a.vc_sh = st[7], a.vc_ss = st[8];
    a.mask = mask, a.m_sb = st[9], a.out = out, a.o_sb = st[10], a.o_sh = st[11];
    a.ws = ws, a.tickets = tickets, a.kv_len_bias = kv_len_bias, a.advance = advance;
    a.S = S, a.groups = H / Hkv, a.scaling = scaling;
    a.stamps = Row::kStamps ? g_attn_stamps : nullptr;
    return dispatch_attn(D, mask != nullptr, S, splits, Row::kBadHeadDim, [&](auto d, auto m, auto l) {
        // (a ring takes no mask -- check_ring --: its MASK forms are never launched and are built as the plain row policy's)
        constexpr bool M = decltype(m)::value, RG = RING && !M;
        launch_kernel(rope_attn_decode_kernel<std::conditional_t<RG, KvF16Ring, Row>, decltype(d)::value, M, decltype(l)::value, PAD, WIN, RG>,
                      dim3(splits, H, B), dim3(kAttnThreads), 0, stream, kv_len, slots, positions, kc, vc, a);
        return check_hip(hipGetLastError(), Row::kOneLaunch);
    });
}

}  // namespace

void set_attn_stamps(unsigned long long* buf) { g_attn_stamps = buf; }

int launch_attn_decode(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv,
                       int S, int D, int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                       int64_t* advance, hipStream_t stream)
{
    return launch_attn<KvF16, false>(q, k, v, {}, mask, out, ws, B, H, Hkv, S, D, splits, scaling, strides, kv_len, kv_len_bias,
                                     advance, stream, NoKvStart{});
}

// launch_attn_decode with a per-row first key: batch row b attends cache rows [kv_start[b], valid length) (DEVICE [B])
int launch_attn_decode_padded(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv,
                              int S, int D, int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                              const int64_t* kv_start, int64_t* advance, hipStream_t stream)
{
    EETQ_REQUIRE(kv_start, "null kv_start");
    return launch_attn<KvF16, true>(q, k, v, {}, mask, out, ws, B, H, Hkv, S, D, splits, scaling, strides, kv_len, kv_len_bias, advance,
                                    stream, kv_start);
}

// the decode entries with a sliding window: batch row b attends the last `window` of its valid rows, not below kv_start[b] (DEVICE
// [B], or nullptr); the bits of the padded entries called with kv_start'[b] = max(kv_start[b], valid length - window)
int launch_attn_decode_window(const f16* q, const f16* k, const f16* v, const f16* mask, f16* out, float* ws, int B, int H, int Hkv,
                              int S, int D, int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias,
                              const int64_t* kv_start, int window, int64_t* advance, hipStream_t stream)
{
    EETQ_REQUIRE(window >= 1, "the attention window must be at least 1 row");
    return launch_attn<KvF16, true, true>(q, k, v, {}, mask, out, ws, B, H, Hkv, S, D, splits, scaling, strides, kv_len, kv_len_bias,
                                          advance, stream, KvWindow{kv_start, window});
}

int launch_rope_attn_decode_window(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                                   const f16* v, const f16* cos_sin, f16* kc, f16* vc, const f16* mask, f16* out, float* ws,
                                   unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                                   const long* st, const int64_t* kv_len, int kv_len_bias, const int64_t* kv_start, int window,
                                   int64_t* advance, long table_rows, hipStream_t stream)
{
    EETQ_REQUIRE(window >= 1, "the attention window must be at least 1 row");
    return launch_rope_attn<KvF16, true, true>(positions, slots, slot_stride, q, k, v, cos_sin, kc, vc, {}, mask, out, ws, tickets, B, H,
                                               Hkv, S, D, splits, scaling, st, kv_len, kv_len_bias, kv_start, advance, table_rows,
                                               stream, window);
}

// the windowed decode entries over a RING cache of S = R rows: logical row r at physical row r mod R, kv_len the logical length; the
// bits of the windowed entries on a static cache that holds the same logical rows.  R >= window, no kv_start, no mask.
int launch_attn_decode_ring(const f16* q, const f16* k, const f16* v, f16* out, float* ws, int B, int H, int Hkv, int S, int D,
                            int splits, float scaling, const long* strides, const int64_t* kv_len, int kv_len_bias, int window,
                            int64_t* advance, hipStream_t stream)
{
    return launch_attn<KvF16, true, true, true>(q, k, v, {}, nullptr, out, ws, B, H, Hkv, S, D, splits, scaling, strides, kv_len,
                                                kv_len_bias, advance, stream, KvWindow{nullptr, window});
}

int launch_rope_attn_decode_ring(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                                 const f16* v, const f16* cos_sin, f16* kc, f16* vc, f16* out, float* ws, unsigned* tickets, int B,
                                 int H, int Hkv, int S, int D, int splits, float scaling, const long* st, const int64_t* kv_len,
                                 int kv_len_bias, int window, int64_t* advance, long table_rows, hipStream_t stream)
{
    return launch_rope_attn<KvF16, true, true, true>(positions, slots, slot_stride, q, k, v, cos_sin, kc, vc, {}, nullptr, out, ws,
                                                     tickets, B, H, Hkv, S, D, splits, scaling, st, kv_len, kv_len_bias, nullptr, advance,
                                                     table_rows, stream, window);
}

int launch_attn_decode_i8(const f16* q, const int8_t* k, const int8_t* v, const f16* scales, const f16* mask, f16* out, float* ws,
                          int B, int H, int Hkv, int S, int D, int splits, float scaling, const long* strides,
                          const long* scale_strides, const int64_t* kv_len, int kv_len_bias, int64_t* advance, hipStream_t stream)
{
    EETQ_REQUIRE(scales && scale_strides, "null pointer");
    const KvI8::Scales sc{const_cast<f16*>(scales), {scale_strides[0], scale_strides[1], scale_strides[2]}};
    return launch_attn<KvI8, false>(q, k, v, sc, mask, out, ws, B, H, Hkv, S, D, splits, scaling, strides, kv_len, kv_len_bias, advance,
                                    stream, NoKvStart{});
}

int launch_rope_attn_decode(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                            const f16* v, const f16* cos_sin, f16* kc, f16* vc, const f16* mask, f16* out, float* ws,
                            unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                            const long* st, const int64_t* kv_len, int kv_len_bias, int64_t* advance, long table_rows,
                            hipStream_t stream)
{
    return launch_rope_attn<KvF16, false>(positions, slots, slot_stride, q, k, v, cos_sin, kc, vc, {}, mask, out, ws, tickets, B, H, Hkv,
                                          S, D, splits, scaling, st, kv_len, kv_len_bias, nullptr, advance, table_rows, stream);
}

// launch_rope_attn_decode with a per-row first key: batch row b attends cache rows [kv_start[b], valid length) (DEVICE [B])
int launch_rope_attn_decode_padded(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                                   const f16* v, const f16* cos_sin, f16* kc, f16* vc, const f16* mask, f16* out, float* ws,
                                   unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                                   const long* st, const int64_t* kv_len, int kv_len_bias, const int64_t* kv_start,
                                   int64_t* advance, long table_rows, hipStream_t stream)
{
    EETQ_REQUIRE(kv_start, "null kv_start");
    return launch_rope_attn<KvF16, true>(positions, slots, slot_stride, q, k, v, cos_sin, kc, vc, {}, mask, out, ws, tickets, B, H, Hkv,
                                         S, D, splits, scaling, st, kv_len, kv_len_bias, kv_start, advance, table_rows, stream);
}

int launch_rope_attn_decode_i8(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                               const f16* v, const f16* cos_sin, int8_t* kc, int8_t* vc, f16* scales, const f16* mask, f16* out,
                               float* ws, unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                               const long* st, const long* scale_strides, const int64_t* kv_len, int kv_len_bias, int64_t* advance,
                               long table_rows, hipStream_t stream)
{
    EETQ_REQUIRE(scales && scale_strides, "null pointer");
    const KvI8::Scales sc{scales, {scale_strides[0], scale_strides[1], scale_strides[2]}};
    return launch_rope_attn<KvI8, false>(positions, slots, slot_stride, q, k, v, cos_sin, kc, vc, sc, mask, out, ws, tickets, B, H, Hkv,
                                         S, D, splits, scaling, st, kv_len, kv_len_bias, nullptr, advance, table_rows, stream);
}

// the dropped-step count of both row formats since the last reset
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
