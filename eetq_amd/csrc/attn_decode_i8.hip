// Decode attention over an int8 KV cache: the kernels of attn_decode.hip on rows of D bytes and one dword of scales per row
// (kv_i8.hpp).  A sibling file rather than a parameter of the fp16 code, so that the fp16 kernels are compiled
// exactly as before.  What changes against attn_decode.hip is the cache element alone:
//   * a lane's share of a row is 8 bytes (one 8-byte load for K, one for V) and the row's scale pair comes with one dword load
//     through a third descriptor that ends at the valid length as well: a row that does not count returns bytes 0, scale 0;
//   * bytes become fp16 pairs by the biased-byte trick (exact integers), q . k8 is summed in fp32 by v_dot2_f32_f16 and the
//     K scale is folded into the score (ks * scaling) * (q . k8), the V scale into the probability: o += (p * vs) * v8;
//     vs * v8 is exact in fp32, so a row that holds all the weight comes out as fp16(vs * v8) bit for bit;
//   * the one-launch form quantises the new token's rotated K and its V in registers, writes bytes and scale pair from one
//     position group per kv head, and every workgroup attends the new row as its quantised self from registers.
// Trips, chunk merge, publish, ticket, head merge and advance are attn_decode_shared.hpp's: both forms give the same bits.
#include "attn_decode_shared.hpp"
#include "kv_i8.hpp"

namespace eetq {
// decode steps of the int8 one-launch form whose new token was not written (cache row outside the cache, negative position)
__device__ unsigned g_attn_i8_dropped = 0;
}  // namespace eetq

namespace eetq {

namespace {

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

template <int D, int U0, int UN, bool MASK, int U>
__device__ __forceinline__ void load_range8(KvBlocks8<U>& t, const KvSrc8& s, int blk0, int dblk, int rib)
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
template <int D, int U, bool MASK>
__device__ __forceinline__ void load_blocks8(KvBlocks8<U>& t, const KvSrc8& s, int blk0, int dblk, int rib)
{
    load_range8<D, 0, U, MASK>(t, s, blk0, dblk, rib);
}

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

// the new token's row as the cache will hold it
struct NewRow8 {
    u32x2 k, v;  // this lane's 8 bytes
    u32   s;     // the row's scale pair
};

// consume_range of attn_decode.hip on int8 rows
template <int D, int U0, int UN, bool SUBST, bool MASK, int U>
__device__ __forceinline__ void consume_range8(KvBlocks8<U>& t, int blk0, int dblk, int rib, int Sv, int slot, const NewRow8& nw,
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

// attn_chunk of attn_decode.hip on int8 rows: the same trips
template <int D, bool SUBST, bool MASK, bool LONG>
__device__ __forceinline__ void attn_chunk8(const f16x8& qv, float scaling, KvBlocks8<kUA>& ta, KvBlocks8<kUB>& tb, const KvSrc8& src,
                                            int split, int splits, int Sv, int slot, const NewRow8& nw, float* sm_m, float* sm_l,
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

    static_assert(kUA == kUB && kUA % kUG == 0, "trip structure");
    const int blk_b = split + kUA * splits;
    auto trips_ab = [&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value;
        load_range8<D, I * kUG, kUG, MASK>(tb, src, blk_b, splits, rib);
        __builtin_amdgcn_sched_barrier(0);
        consume_range8<D, I * kUG, kUG, SUBST, MASK>(ta, split, splits, rib, Sv, slot, nw, q2, scaling, m, l, o);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto trips_b = [&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value;
        consume_range8<D, I * kUG, kUG, SUBST, MASK>(tb, blk_b, splits, rib, Sv, slot, nw, q2, scaling, m, l, o);
    };
    constexpr int NT = kUA / kUG;
    static_for<NT>(trips_ab);
    if constexpr (LONG) {
        const int      nblk = (Sv + BLK - 1) / BLK;
        int            ub   = kUA + kUB;
        KvBlocks8<kUL> tl, tn;
        load_blocks8<D, kUL, MASK>(tl, src, split + ub * splits, splits, rib);
        __builtin_amdgcn_sched_barrier(0);
        static_for<NT>(trips_b);
        while (split + ub * splits < nblk) {  // workgroup-uniform
            load_blocks8<D, kUL, MASK>(tn, src, split + (ub + kUL) * splits, splits, rib);
            consume_range8<D, 0, kUL, SUBST, MASK>(tl, split + ub * splits, splits, rib, Sv, slot, nw, q2, scaling, m, l, o);
            tl = tn;
            ub += kUL;
        }
    } else {
        static_for<NT>(trips_b);
    }

    chunk_merge<D>(m, l, o, sm_m, sm_l, sm_o, M, L, O);
}

// the buffer descriptors of one (batch row, kv head), all three ending at the valid length Sv; strides in bytes (k, v) and
// fp16 elements (scales)
template <int D, bool MASK>
__device__ __forceinline__ KvSrc8 make_kv_src8(const int8_t* kbase, const int8_t* vbase, const f16* sbase, long k_ss, long v_ss,
                                               long s_ss, int Sv, const f16* mrow)
{
    KvSrc8 s;
    s.k_row = (unsigned)k_ss;
    s.v_row = (unsigned)v_ss;
    s.s_row = (unsigned)(s_ss * 2);
    s.d0b   = (unsigned)(((threadIdx.x & 63) % AttnGeo<D>::LPP) * 8);
    s.k = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(kbase), 0, (int)((unsigned)Sv * s.k_row), 0x00020000);
    s.v = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(vbase), 0, (int)((unsigned)Sv * s.v_row), 0x00020000);
    s.s = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(sbase), 0, (int)((unsigned)Sv * s.s_row), 0x00020000);
    s.m = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(MASK ? mrow : sbase), 0, MASK ? Sv * 2 : 0, 0x00020000);
    return s;
}

struct ScaleStrides {
    long sb, sh, ss;  // fp16 elements between batch rows, kv heads, rows of the scale tensor
};

template <int D, bool MASK, bool LONG>
__global__ __launch_bounds__(kAttnThreads) void attn_decode_partial_i8_kernel(
    const f16* __restrict__ q, const int8_t* __restrict__ kc, const int8_t* __restrict__ vc, const f16* __restrict__ scales,
    const f16* __restrict__ mask, float* __restrict__ ws, float scaling, int S, int groups, long q_sb, long q_sh, long k_sb,
    long k_sh, long k_ss, long v_sb, long v_sh, long v_ss, long m_sb, ScaleStrides sst, const int64_t* __restrict__ kv_len,
    int kv_len_bias)
{
    constexpr int NW = kAttnThreads / 64;
    __shared__ float sm_m[NW], sm_l[NW];
    __shared__ __attribute__((aligned(16))) float sm_o[NW * D];

    const int split = blockIdx.x, splits = gridDim.x, h = blockIdx.y, b = blockIdx.z, hk = h / groups;
    const int tid = threadIdx.x, d0 = ((tid & 63) % (D / 8)) * 8;
    const int rib = (tid >> 6) * AttnGeo<D>::PPW + (tid & 63) / AttnGeo<D>::LPP;
    const int Sv = valid_len(S, kv_len, kv_len_bias);

    const f16x8  qv  = *reinterpret_cast<const f16x8*>(q + b * q_sb + h * q_sh + d0);
    const KvSrc8 src = make_kv_src8<D, MASK>(kc + b * k_sb + hk * k_sh, vc + b * v_sb + hk * v_sh, scales + b * sst.sb + hk * sst.sh,
                                             k_ss, v_ss, sst.ss, Sv, MASK ? mask + b * m_sb : nullptr);
    KvBlocks8<kUA> ta;
    KvBlocks8<kUB> tb;
    load_blocks8<D, kUA, MASK>(ta, src, split, splits, rib);
    float         M, L, O;
    const NewRow8 none = {};
    attn_chunk8<D, false, MASK, LONG>(qv, scaling, ta, tb, src, split, splits, Sv, -1, none, sm_m, sm_l, sm_o, M, L, O);
    if (tid < D) {
        float* out = ws + (((size_t)b * gridDim.x + split) * gridDim.y + h) * (D + kRecPad);  // [batch][split][head][record]
        out[kRecPad + tid] = O;
        if (tid == 0) {
            out[0] = M;
            out[1] = L;
        }
    }
}

struct RopeAttnArgs8 {
    RopeAttnArgs a;  // kc_* / vc_* strides in bytes
    f16*         scales;
    ScaleStrides sst;
};

// rope_attn_decode_kernel of attn_decode.hip on an int8 cache; grid (splits, heads, batch), 256 threads
template <int D, bool MASK, bool LONG>
__global__ __launch_bounds__(kAttnThreads) void rope_attn_decode_i8_kernel(const int64_t* __restrict__ kv_len,
                                                                           const int64_t* __restrict__ slots,
                                                                           const int64_t* __restrict__ positions,
                                                                           int8_t* __restrict__ kc, int8_t* __restrict__ vc,
                                                                           const RopeAttnArgs8 x)
{
    constexpr int LPP = D / 8, NW = kAttnThreads / 64;
    __shared__ float    sm_m[NW], sm_l[NW];
    __shared__ __attribute__((aligned(16))) float sm_o[NW * D];
    __shared__ unsigned sm_ticket;

    const RopeAttnArgs& a = x.a;
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z, hk = h / a.groups;
    const int splits = gridDim.x, H = gridDim.y;
    const int tid = threadIdx.x, lane = tid & 63, li = lane % LPP, d0 = li * 8;
    const int d1 = d0 < D / 2 ? d0 + D / 2 : d0 - D / 2;  // the paired channels of the rotation

    // the three scalar reads of the fp16 kernel, as one batch
    const int64_t* p_pos  = positions + b;
    const int64_t* p_slot = slots ? slots + (long)b * a.slot_stride : positions + b;
    const int64_t* p_len  = kv_len ? kv_len : positions;
    int64_t        rpos, slot64, filled;
    asm volatile("s_load_dwordx2 %0, %3, 0x0\n\ts_load_dwordx2 %1, %4, 0x0\n\ts_load_dwordx2 %2, %5, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(rpos), "=&s"(slot64), "=&s"(filled)
                 : "s"(p_pos), "s"(p_slot), "s"(p_len)
                 : "memory");
    // a slot outside the cache is neither written nor attended, and nothing is rotated then
    const bool have_new = slot64 >= 0 && slot64 < a.S && rpos >= 0;
    const int  slot = have_new ? (int)slot64 : -1;
    if (!have_new && split == 0 && h == 0 && threadIdx.x == 0) atomicAdd(&g_attn_i8_dropped, 1u);
    const int  Sv = kv_len ? max(0, (int)min((int64_t)a.S, filled + a.kv_len_bias)) : a.S;

    // the new token and its cos | sin row first, then the chunk's first kUA blocks
    const f16*  qp = a.q + b * a.q_sb + (long)h * D;
    const f16*  kp = a.k + b * a.k_sb + (long)hk * D;
    f16x8       qv   = *reinterpret_cast<const f16x8*>(qp + d0);
    f16x8       knew = *reinterpret_cast<const f16x8*>(kp + d0);
    const f16x8 vnew = *reinterpret_cast<const f16x8*>(a.v + b * a.v_sb + (long)hk * D + d0);
    const f16x8 qpair = *reinterpret_cast<const f16x8*>(qp + d1), kpair = *reinterpret_cast<const f16x8*>(kp + d1);
    const f16*  cs = a.cos_sin + (have_new ? rpos : 0) * D + (d0 < D / 2 ? d0 : d0 - D / 2);
    const f16x8 rc = *reinterpret_cast<const f16x8*>(cs), rs = *reinterpret_cast<const f16x8*>(cs + D / 2);
    __builtin_amdgcn_sched_barrier(0);
    const KvSrc8 src = make_kv_src8<D, MASK>(kc + b * a.kc_sb + hk * a.kc_sh, vc + b * a.vc_sb + hk * a.vc_sh,
                                             x.scales + b * x.sst.sb + hk * x.sst.sh, a.kc_ss, a.vc_ss, x.sst.ss, Sv,
                                             MASK ? a.mask + b * a.m_sb : nullptr);
    const int    rib = (tid >> 6) * AttnGeo<D>::PPW + lane / LPP;
    KvBlocks8<kUA> ta;
    KvBlocks8<kUB> tb;
    load_blocks8<D, kUA, MASK>(ta, src, split, splits, rib);
    __builtin_amdgcn_sched_barrier(0);
    if (have_new) {
        qv   = rope8<D>(qv, qpair, rc, rs, d0);
        knew = rope8<D>(knew, kpair, rc, rs, d0);
    }
    // the row as the cache holds it: every position group of every workgroup has the whole row across its LPP lanes
    NewRow8 nw;
    {
        const f16 ks = kv8_scale(group_max<LPP>(kv8_abs_max8(knew))), vs = kv8_scale(group_max<LPP>(kv8_abs_max8(vnew)));
        nw.k = kv8_quant8(knew, ks);
        nw.v = kv8_quant8(vnew, vs);
        nw.s = as_u32(f16x2{ks, vs});
    }
    __builtin_amdgcn_sched_barrier(0);
    // the cache row of the new token: once per kv head, by one position group of the head's first workgroup
    if (have_new && split == 0 && h == hk * a.groups && tid < LPP) {
        *reinterpret_cast<u32x2*>(kc + b * a.kc_sb + hk * a.kc_sh + (long)slot * a.kc_ss + d0) = nw.k;
        *reinterpret_cast<u32x2*>(vc + b * a.vc_sb + hk * a.vc_sh + (long)slot * a.vc_ss + d0) = nw.v;
        if (tid == 0) *reinterpret_cast<u32*>(x.scales + b * x.sst.sb + hk * x.sst.sh + (long)slot * x.sst.ss) = nw.s;
    }
    float M, L, O;
    attn_chunk8<D, true, MASK, LONG>(qv, a.scaling, ta, tb, src, split, splits, Sv, slot, nw, sm_m, sm_l, sm_o, M, L, O);
    head_handoff<D>(a, split, splits, h, b, H, M, L, O, sm_o, &sm_ticket);
}

template <int D, bool MASK, bool LONG>
int launch_d2_i8(const f16* q, const int8_t* k, const int8_t* v, const f16* scales, const f16* mask, f16* out, float* ws, int B, int H,
                 int Hkv, int S, int splits, float scaling, const long* st, const ScaleStrides& sst, const int64_t* kv_len,
                 int kv_len_bias, int64_t* advance, hipStream_t stream)
{
    launch_kernel(attn_decode_partial_i8_kernel<D, MASK, LONG>, dim3(splits, H, B), dim3(kAttnThreads), 0, stream, q, k, v, scales,
                  mask, ws, scaling, S, H / Hkv, st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], st[8], sst, kv_len,
                  kv_len_bias);
    EETQ_TRY_HIP(hipGetLastError());
    launch_kernel(attn_decode_merge_kernel<D>, dim3(H, B), dim3(kAttnThreads), 0, stream, (const float*)ws, out, splits, st[9],
                  st[10], advance);
    return check_hip(hipGetLastError(), "attn_decode_i8 kernels launch");
}

template <int D>
int launch_d_i8(const f16* q, const int8_t* k, const int8_t* v, const f16* scales, const f16* mask, f16* out, float* ws, int B, int H,
                int Hkv, int S, int splits, float scaling, const long* st, const ScaleStrides& sst, const int64_t* kv_len,
                int kv_len_bias, int64_t* advance, hipStream_t stream)
{
    const bool lng = long_chunks<D>(S, splits);
#define EETQ_ATTN_GO(MASK, LONG)                                                                                                  \
    return launch_d2_i8<D, MASK, LONG>(q, k, v, scales, mask, out, ws, B, H, Hkv, S, splits, scaling, st, sst, kv_len, kv_len_bias, \
                                       advance, stream)
    if (mask) {
        if (lng) EETQ_ATTN_GO(true, true);
        EETQ_ATTN_GO(true, false);
    }
    if (lng) EETQ_ATTN_GO(false, true);
    EETQ_ATTN_GO(false, false);
#undef EETQ_ATTN_GO
}

template <int D>
int launch_rope_d_i8(const int64_t* kv_len, const int64_t* slots, const int64_t* positions, int8_t* kc, int8_t* vc,
                     const RopeAttnArgs8& x, dim3 grid, hipStream_t stream)
{
    const bool lng = long_chunks<D>(x.a.S, (int)grid.x);
#define EETQ_ATTN_GO(MASK, LONG) \
    launch_kernel(rope_attn_decode_i8_kernel<D, MASK, LONG>, grid, dim3(kAttnThreads), 0, stream, kv_len, slots, positions, kc, vc, x)
    if (x.a.mask) {
        if (lng) EETQ_ATTN_GO(true, true);
        else EETQ_ATTN_GO(true, false);
    } else {
        if (lng) EETQ_ATTN_GO(false, true);
        else EETQ_ATTN_GO(false, false);
    }
#undef EETQ_ATTN_GO
    return check_hip(hipGetLastError(), "rope_attn_decode_i8_kernel launch");
}

}  // namespace

int launch_attn_decode_i8(const f16* q, const int8_t* k, const int8_t* v, const f16* scales, const f16* mask, f16* out, float* ws,
                          int B, int H, int Hkv, int S, int D, int splits, float scaling, const long* strides,
                          const long* scale_strides, const int64_t* kv_len, int kv_len_bias, int64_t* advance, hipStream_t stream)
{
    EETQ_REQUIRE(q && k && v && scales && out && ws && strides && scale_strides, "null pointer");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && S > 0 && splits > 0 && splits <= S, "invalid attention shape");
    EETQ_REQUIRE(strides[0] % 8 == 0 && strides[1] % 8 == 0, "q strides must be multiples of 8 elements (16-byte loads)");
    EETQ_REQUIRE((uintptr_t)q % 16 == 0, "q must be 16-byte aligned");
    const int st = check_i8_cache(k, v, scales, S, strides + 2, scale_strides);
    if (st != EETQ_OK) return st;
    const ScaleStrides sst{scale_strides[0], scale_strides[1], scale_strides[2]};
    if (D == 128)
        return launch_d_i8<128>(q, k, v, scales, mask, out, ws, B, H, Hkv, S, splits, scaling, strides, sst, kv_len, kv_len_bias,
                                advance, stream);
    if (D == 64)
        return launch_d_i8<64>(q, k, v, scales, mask, out, ws, B, H, Hkv, S, splits, scaling, strides, sst, kv_len, kv_len_bias,
                               advance, stream);
    return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] decode attention on an int8 cache supports head_dim 64 and 128");
}

int launch_rope_attn_decode_i8(const int64_t* positions, const int64_t* slots, int slot_stride, const f16* q, const f16* k,
                               const f16* v, const f16* cos_sin, int8_t* kc, int8_t* vc, f16* scales, const f16* mask, f16* out,
                               float* ws, unsigned* tickets, int B, int H, int Hkv, int S, int D, int splits, float scaling,
                               const long* st, const long* scale_strides, const int64_t* kv_len, int kv_len_bias, int64_t* advance,
                               long table_rows, hipStream_t stream)
{
    EETQ_REQUIRE(positions && q && k && v && cos_sin && kc && vc && scales && out && ws && tickets && st && scale_strides,
                 "null pointer");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && S > 0 && splits > 0 && splits <= S && splits <= 4096,
                 "invalid attention shape");
    EETQ_REQUIRE(slot_stride == 0 || slot_stride == 1, "slot_stride must be 0 (one slot for the batch) or 1");
    // validated, not enforced on the device: as in the fp16 entry
    EETQ_REQUIRE(table_rows > 0, "the cos|sin table must have at least one row");
    for (int i = 0; i < 3; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q / k / v strides must be multiples of 8 elements (16-byte accesses)");
    EETQ_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)cos_sin) % 16 == 0,
                 "q, k, v and the cos|sin table must be 16-byte aligned");
    const int cs = check_i8_cache(kc, vc, scales, S, st + 3, scale_strides);
    if (cs != EETQ_OK) return cs;
    RopeAttnArgs8 x;
    RopeAttnArgs& a = x.a;
    a.slot_stride = slot_stride;
    a.q = q, a.k = k, a.v = v, a.q_sb = st[0], a.k_sb = st[1], a.v_sb = st[2];
    a.cos_sin = cos_sin;
    a.kc_sb = st[3], a.kc_sh = st[4], a.kc_ss = st[5], a.vc_sb = st[6], a.vc_sh = st[7], a.vc_ss = st[8];
    a.mask = mask, a.m_sb = st[9], a.out = out, a.o_sb = st[10], a.o_sh = st[11];
    a.ws = ws, a.tickets = tickets, a.kv_len_bias = kv_len_bias, a.advance = advance;
    a.S = S, a.groups = H / Hkv, a.scaling = scaling;
    a.stamps = nullptr;
    x.scales = scales;
    x.sst    = ScaleStrides{scale_strides[0], scale_strides[1], scale_strides[2]};
    if (D == 128) return launch_rope_d_i8<128>(kv_len, slots, positions, kc, vc, x, dim3(splits, H, B), stream);
    if (D == 64) return launch_rope_d_i8<64>(kv_len, slots, positions, kc, vc, x, dim3(splits, H, B), stream);
    return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] decode attention on an int8 cache supports head_dim 64 and 128");
}

int attn_i8_dropped_steps(unsigned* count, bool reset)
{
    EETQ_TRY_HIP(hipMemcpyFromSymbol(count, HIP_SYMBOL(g_attn_i8_dropped), sizeof(unsigned)));
    if (reset) {
        const unsigned zero = 0;
        EETQ_TRY_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_attn_i8_dropped), &zero, sizeof(unsigned)));
    }
    return EETQ_OK;
}

}  // namespace eetq
