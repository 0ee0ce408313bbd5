// Few-row attention behind a long cache: R = 1 .. 16 query rows per batch row -- the rows a static fp16 KV cache has just been
// given (a speculative verify step's k + 1 rows, a chunked prompt's short last piece) -- attending the cache causally among
// themselves, split-KV, both products on v_mfma_f32_16x16x32_f16.  Semantics: eetq_prefill_attention_dev_f16's.
//
// The prompt kernel (attn_prefill.hip) gives such a call 128-row workgroups of which 2 .. 16 rows are real, at most 16 shares of
// the keys and one stream of the K / V rows per QUERY head; the decode kernel (attn_decode.hip) has the right shape -- many chunks
// per head, the cache read once -- but is a VALU dot product for one row.  Here:
//
//   work      one workgroup (4 waves) per (chunk of the keys, kv head, batch row).  The groups * R (head of the group, query row)
//             pairs of a kv head form ONE query tile, so a K / V row is loaded once per kv head; the tile is cut into 16-row
//             sub-tiles (NSUB = 1 .. 4 of them in registers; a tile of more than 64 rows -- more than 4 heads per kv head at 16
//             rows -- takes further workgroups, grid.y, which stream the rows again).
//   keys      in BLOCKS of kRowsBlk = 32 rows.  Chunk i of `splits` owns blocks [i nblk / splits, (i + 1) nblk / splits) of the
//             nblk = ceil(keys / 32) blocks (integer division: the closed formula of the header); wave w takes the chunk's blocks
//             w, w + 4, ...  All waves run the same number of trips (the barriers are workgroup barriers); a wave without a block
//             in a trip requests nothing (its offsets are out of the descriptors' range) and computes nothing.
//   S^T       = K Q^T per 16 keys: the K rows are the A operand STRAIGHT from global memory (lane = key lane & 15, channels
//             32 ks + 8 (lane >> 4) ..: one 16-byte load per k-step), the sub-tile's Q rows the B operand, held in registers.
//             A lane then owns ONE query column and keys 4 (lane >> 4) + i of the 16: maximum and sum are 7 local operations and
//             two lane swaps, and the probabilities -- rounded to fp16, carried as 2^12 p (kAttnPShift of common.hpp and the
//             comment there) -- ARE the B operand of the second product: k-slots 8 g + i = key 4 g + i of the first 16-key group,
//             8 g + 4 + i = the same of the second.
//   O^T       += V^T P^T per 32 keys: V goes through a wave-private transposed LDS image ([channel][32 keys], 72-byte pitch; a
//             lane holds one 16-byte chunk of four consecutive rows and writes four keys of one channel at a time), read back as two
//             8-byte pieces per 16 channels in the k-slot order above.  The image is shared by the tile's sub-tiles.
//   loads     unconditional buffer loads, nt, through descriptors that END AT THE VALID LENGTH (attn_decode_shared.hpp): rows at
//             and beyond `keys` read as zeros and are never touched.  The row offset rides in the VECTOR offset, the scalar offset
//             is zero (a scalar offset beyond num_records can wrap).  The causal tail lies inside the valid length: it
//             is masked by select on the score, -inf contributing exactly zero.  Block j + 1 is requested before block j is used.
//   records   the waves' states meet in LDS (in wave order: deterministic), and every chunk writes, per (query row, head), the
//             record [m, l, -, -, o[D]] (kRecPad) -- an empty chunk or a row with nothing to attend in it (-inf, 0, zeros): the
//             workspace's earlier contents never matter.  attn_rows_merge_kernel, a second launch, weights a row's records by
//             exp2(m_i - max m) and divides once; a fully masked row gives zeros.  No tickets, no atomics, no state between launches.
//
// KV8 (the int8 row format of kv_i8.hpp; eetq_decode_attention_rows_i8kv_f16): the same work, chunks, blocks, sub-tiles, records and
// merge over int8 rows, in the arithmetic of eetq_prefill_attention_i8kv_f16.  What changes is fetch, the A operand and stage:
//   * a lane's share of a K row per k-step and of a V row per chunk is 8 BYTES (the same channels, strides in bytes), and lane l of a
//     wave also loads the scale dword (k scale, v scale) of key l & 31 of the block through a third descriptor that ends at the valid
//     length like the other two: a row at or beyond `keys` reads as bytes 0, scales 0, whatever memory holds there;
//   * the K bytes become the A operand as exact fp16 integers (kv8_unpack8), once per block for all sub-tiles, and the K scale is
//     folded into the fp32 score behind the product, per key, before the mask select: x = (ks * scaling log2 e) * (q . k8).  The eight
//     scales of a lane's keys 4 (lane >> 4) + i of both 16-key groups come from the owning lanes by lane read (ds_bpermute);
//   * a V row enters the transposed image as fp16(vs * v8): one packed fp16 multiply of the exact integer by the row's scale (read
//     from the lane that holds the row's dword), one rounding of the exact product, denormals kept -- not vs riding on the
//     probability.  The image, its pitch and the fragments read from it are the fp16 form's.
#include "attn_decode_shared.hpp"
#include "kv_i8.hpp"

namespace eetq {

namespace {

constexpr int   kRowsThreads = 256, kRowsWaves = 4;
constexpr int   kRowsBlk = 32;          // keys per block (one wave, one trip)
constexpr int   kRowsMaxR = 16;         // query rows per batch row
constexpr int   kRowsMaxSub = 4;        // 16-row sub-tiles a workgroup holds
constexpr int   kRowsMaxSplits = 64;
constexpr int   kRowsVtPitch = kRowsBlk + 4;   // halfs per channel row of the transposed V image (72 bytes)

struct RowsArgs {
    const f16*     q;
    const f16*     k;
    const f16*     v;
    float*         ws;
    long           q_sb, q_st, q_sh, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;
    const int64_t* kv_len;   // DEVICE scalar or nullptr
    int            kv_len_bias, max_keys, R, H, groups, ntg;
    float          c;        // scaling * log2(e)
};
// KV8: k and v point at int8 rows, their strides are in BYTES, and the rows' scale pairs lie in `scales`.  Behind the fp16 form's
// arguments, which keep their kernarg block.
struct RowsArgs8 : RowsArgs {
    const f16* scales;
    long       s_sb, s_sh, s_ss;   // fp16 elements between batch rows, kv heads, rows of the scale tensor
};
template <bool KV8>
using RowsKernArgs = std::conditional_t<KV8, RowsArgs8, RowsArgs>;

// the value of lane ^ 16 and lane ^ 32 folded in: every lane of a query column ends with the column's maximum / sum
__device__ __forceinline__ float col_max(float v)
{
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float col_sum(float v)
{
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// grid (splits, kv heads * ntg, batch)
template <int D, int NSUB, bool KV8 = false>
__global__ __launch_bounds__(kRowsThreads) void attn_rows_partial_kernel(const RowsKernArgs<KV8> a)
{
    static_assert(D == 128 || D == 64, "head_dim 128 or 64");
    constexpr int KS = D / 32;                      // k-steps of the score product
    constexpr int CT = D / 16;                      // 16-channel tiles of the output
    constexpr int CH = D / 8;                       // 16-byte chunks per row (KV8: 8-byte chunks, the same channels)
    constexpr int PG = 64 / CH;                     // lane groups of the V staging (4 or 8), four rows each
    constexpr int NQ = kRowsBlk / (4 * PG);         // quads of rows per lane (2 or 1)
    constexpr int REC = D + kRecPad;
    constexpr int VT_WAVE = D * kRowsVtPitch;       // halfs of one wave's image
    // the V images (4 x 9 216 bytes at D = 128) and, after the loop, the tile's records (64 x 528 bytes) share one buffer
    constexpr int LDS_BYTES = kRowsWaves * VT_WAVE * 2 > 16 * NSUB * REC * 4 ? kRowsWaves * VT_WAVE * 2 : 16 * NSUB * REC * 4;
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[LDS_BYTES];
    __shared__ float sm_m[kRowsWaves][16 * NSUB];

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, ln = lane & 15, g4 = lane >> 4;
    const int split = blockIdx.x, splits = gridDim.x, b = blockIdx.z;
    const int hk = (int)blockIdx.y / a.ntg, tg = (int)blockIdx.y % a.ntg;

    int keys = a.max_keys;
    if (a.kv_len) {
        const int64_t n = *a.kv_len + (int64_t)a.kv_len_bias;   // uniform: a scalar load
        keys = (int)max((int64_t)0, min((int64_t)a.max_keys, n));
    }
    const int koff = keys - a.R;
    const int nblk = (keys + kRowsBlk - 1) / kRowsBlk;
    const int j0 = (int)((long)split * nblk / splits), j1 = (int)((long)(split + 1) * nblk / splits);
    const int trips = (j1 - j0 + kRowsWaves - 1) / kRowsWaves;

    // ---- the tile's rows: row r = head-of-group * R + query row; rows beyond the tile are clamped on the way in and never stored ----
    const int tile_rows = a.groups * a.R, row0 = tg * 16 * kRowsMaxSub;
    int       qt[NSUB];   // this lane's query row (its causal limit) per sub-tile
    f16x8     qf[NSUB][KS];
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        const int r = min(row0 + 16 * s + ln, tile_rows - 1), g = r / a.R;
        qt[s] = r - g * a.R;
        const f16* qp = a.q + b * a.q_sb + (long)qt[s] * a.q_st + (long)(hk * a.groups + g) * a.q_sh + 8 * g4;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[s][ks] = *reinterpret_cast<const f16x8*>(qp + 32 * ks);
    }

    // ---- the valid rows of this (batch row, kv head) behind descriptors ----
    // (KV8: the same two with strides in bytes, and the rows' scale dwords behind a third one)
    constexpr unsigned EB = KV8 ? 1u : 2u;     // bytes per unit of the cache strides and per channel
    const unsigned krow_b = (unsigned)a.k_ss * EB, vrow_b = (unsigned)a.v_ss * EB;
    using CacheElem = std::conditional_t<KV8, int8_t, f16>;
    const CacheElem* kbase = reinterpret_cast<const CacheElem*>(a.k) + b * a.k_sb + hk * a.k_sh;
    const CacheElem* vbase = reinterpret_cast<const CacheElem*>(a.v) + b * a.v_sb + hk * a.v_sh;
    const __amdgpu_buffer_rsrc_t krs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<CacheElem*>(kbase), 0, (int)((unsigned)keys * krow_b), 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<CacheElem*>(vbase), 0, (int)((unsigned)keys * vrow_b), 0x00020000);
    __amdgpu_buffer_rsrc_t srs = krs;          // fp16 rows: not used
    unsigned               srow_b = 0;
    if constexpr (KV8) {
        srow_b = (unsigned)a.s_ss * 2u;
        srs    = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(a.scales + b * a.s_sb + hk * a.s_sh), 0, (int)((unsigned)keys * srow_b),
                                                   0x00020000);
    }
    constexpr unsigned kNoRow = 0x80000000u;   // an offset beyond every descriptor (they span < 2 GiB; no 32-bit wrap): zeros, nothing read

    using CacheReg = std::conditional_t<KV8, u32x2, u32x4>;   // a lane's 8 channels of one row
    CacheReg  kc[2][KS], kn[2][KS], vreg[NQ][4];
    u32       sc8 = 0u, sn8 = 0u;               // KV8: the scale dword of key (lane & 31) of the current / the next block
    const int vc = lane % CH, vp = lane / CH;   // V staging: chunk and row group of this lane
    auto load8 = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned off) {
        if constexpr (KV8) return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, kNt));
        else return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, kNt));
    };
    auto fetch = [&](CacheReg (&kd)[2][KS], u32& sd, int blk) {
        const bool have = blk < j1;             // wave-uniform
        const unsigned key0 = (unsigned)blk * kRowsBlk;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const unsigned row = key0 + 16 * kb + ln;
                const unsigned off = have && row < (unsigned)keys ? row * krow_b + (32 * ks + 8 * g4) * EB : kNoRow;
                kd[kb][ks] = load8(krs, off);
            }
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned row = key0 + qd * 4 * PG + 4 * vp + r;
                const unsigned off = have && row < (unsigned)keys ? row * vrow_b + vc * 8 * EB : kNoRow;
                vreg[qd][r] = load8(vrs, off);
            }
        if constexpr (KV8) {
            const unsigned row = key0 + (lane & 31);
            sd = __builtin_amdgcn_raw_buffer_load_b32(srs, (int)(have && row < (unsigned)keys ? row * srow_b : kNoRow), 0, kNt);
        }
    };
    f16* vt = reinterpret_cast<f16*>(lds_raw) + wave * VT_WAVE;   // this wave's image: [channel][32 keys]
    // a staged row's 8 channels as fp16; KV8: fp16(vs * v8), the row's scale from the lane that holds its dword (all lanes call)
    auto vchunk = [&](int qd, int r, u32 sd) {
        if constexpr (KV8) {
            f16x2 h[4];
            kv8_unpack8(vreg[qd][r], h);
            const f16   vs  = as_f16x2((u32)__shfl((int)sd, qd * 4 * PG + 4 * vp + r, 64))[1];
            const f16x2 vs2 = {vs, vs};
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = h[i] * vs2;   // one rounding of the exact product
            return f16x8{h[0][0], h[0][1], h[1][0], h[1][1], h[2][0], h[2][1], h[3][0], h[3][1]};
        } else {
            return __builtin_bit_cast(f16x8, vreg[qd][r]);
        }
    };
    auto stage = [&](u32 sd) {
#pragma unroll
        for (int qd = 0; qd < NQ; ++qd) {
            const f16x8 v0 = vchunk(qd, 0, sd), v1 = vchunk(qd, 1, sd);
            const f16x8 v2 = vchunk(qd, 2, sd), v3 = vchunk(qd, 3, sd);
            f16*        vw = vt + 8 * vc * kRowsVtPitch + qd * 4 * PG + 4 * vp;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const f16x2 lo = {v0[e], v1[e]}, hh = {v2[e], v3[e]};
                *reinterpret_cast<u32x2*>(vw + e * kRowsVtPitch) = u32x2{as_u32(lo), as_u32(hh)};
            }
        }
    };

    f32x4 o[NSUB][CT];
    float m_run[NSUB], l_run[NSUB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        m_run[s] = -INFINITY, l_run[s] = 0.f;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[s][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    if (trips > 0) {   // workgroup-uniform
        fetch(kc, sc8, j0 + wave);
        stage(sc8);
    }
    __syncthreads();
    for (int it = 0; it < trips; ++it) {
        const int  blk  = j0 + it * kRowsWaves + wave;
        const bool next = it + 1 < trips;           // workgroup-uniform
        if (next) fetch(kn, sn8, blk + kRowsWaves);   // V of block j goes to registers that `stage` has emptied
        if (blk < j1) {                             // wave-uniform
            const int key0 = blk * kRowsBlk;
            // the image's fragments, shared by the sub-tiles: channels 16 ct + ln, keys 4 g4 .. + 3 and 16 + 4 g4 .. + 3
            f16x8 vf[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const f16*  vr = vt + (16 * ct + ln) * kRowsVtPitch + 4 * g4;
                const u32x2 lo = *reinterpret_cast<const u32x2*>(vr), hh = *reinterpret_cast<const u32x2*>(vr + 16);
                vf[ct] = __builtin_bit_cast(f16x8, u32x4{lo.x, lo.y, hh.x, hh.y});
            }
            // KV8: the block's A operands as exact integers, and the K scales of this lane's keys times scaling log2 e
            f16x8 kf[KV8 ? 2 : 1][KV8 ? KS : 1];
            float kx[8];
            if constexpr (KV8) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        f16x2 h[4];
                        kv8_unpack8(kc[kb][ks], h);
                        kf[kb][ks] = f16x8{h[0][0], h[0][1], h[1][0], h[1][1], h[2][0], h[2][1], h[3][0], h[3][1]};
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        kx[4 * kb + i] = (float)as_f16x2((u32)__shfl((int)sc8, 16 * kb + 4 * g4 + i, 64))[0] * a.c;
                }
            }
            auto kfrag = [&](int kb, int ks) {
                if constexpr (KV8) return kf[kb][ks];
                else return __builtin_bit_cast(f16x8, kc[kb][ks]);
            };
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
                // ---- S^T = K Q^T: two 16-key groups ----
                f32x4 sc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
                        sc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfrag(kb, ks), qf[s][ks], sc[kb], 0, 0, 0);
                // ---- scaled scores, masked by select: key < keys and key <= koff + query row ----
                const int lim = min(keys - 1, koff + qt[s]);
                float     x[8], mloc = -INFINITY;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int key = key0 + 16 * kb + 4 * g4 + i;
                        float xs;
                        if constexpr (KV8) xs = kx[4 * kb + i] * sc[kb][i];
                        else xs = sc[kb][i] * a.c;
                        x[4 * kb + i] = key <= lim ? xs : -INFINITY;
                        mloc = fmaxf(mloc, x[4 * kb + i]);
                    }
                mloc = col_max(mloc) - kAttnPShift;                          // the maxima are kept 12 below: p as 2^12 p
                const float m_new = fmaxf(m_run[s], mloc);
                const float m_use = m_new > -INFINITY ? m_new : 0.f;         // a row with nothing to attend yet: every p = 0
                const float alpha = __builtin_amdgcn_exp2f(m_run[s] - m_use);   // exp2(-inf) = 0 for the first block
                float       psum = 0.f;
                f16x8       pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float p = __builtin_amdgcn_exp2f(x[e] - m_use);
                    psum += p;
                    pf[e] = (f16)p;
                }
                l_run[s] = l_run[s] * alpha + col_sum(psum);
                m_run[s] = m_new;
                // ---- O^T = alpha O^T + V^T P^T ----
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    o[s][ct] *= alpha;
                    o[s][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[ct], pf, o[s][ct], 0, 0, 0);
                }
            }
        }
        if (next) {
            __syncthreads();   // the image has been read
            stage(sn8);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) kc[kb][ks] = kn[kb][ks];
            sc8 = sn8;
            __syncthreads();   // the next image is complete
        }
    }

    // ---- the waves' states -> the chunk's records, in LDS: lane (ln, g4) holds row ln of each sub-tile, channels 16 ct + 4 g4 .. + 3 ----
    if (g4 == 0) {
#pragma unroll
        for (int s = 0; s < NSUB; ++s) sm_m[wave][16 * s + ln] = m_run[s];
    }
    __syncthreads();   // (also: every wave is done with its V image, the buffer becomes the records)
    float* rec = reinterpret_cast<float*>(lds_raw);
    float  f[NSUB];
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
        float M = sm_m[0][16 * s + ln];
#pragma unroll
        for (int w = 1; w < kRowsWaves; ++w) M = fmaxf(M, sm_m[w][16 * s + ln]);
        f[s] = __builtin_amdgcn_exp2f(m_run[s] - (M > -INFINITY ? M : 0.f));   // 0 for a wave that attended nothing
        if (wave == 0 && g4 == 0) rec[(16 * s + ln) * REC] = M;
    }
    for (int w = 0; w < kRowsWaves; ++w) {   // wave by wave: a fixed order of the sums
        if (wave == w) {
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
                float* rp = rec + (16 * s + ln) * REC;
                if (g4 == 0) rp[1] = (w == 0 ? 0.f : rp[1]) + l_run[s] * f[s];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    f32x4*      op  = reinterpret_cast<f32x4*>(rp + kRecPad + 16 * ct + 4 * g4);
                    const f32x4 add = o[s][ct] * f[s];
                    *op = w == 0 ? add : *op + add;
                }
            }
        }
        __syncthreads();
    }
    // ---- records -> workspace [batch][head][query row][split][REC], 16 bytes per thread and step ----
    constexpr int F4 = REC / 4;
    const int     nrows = min(16 * NSUB, tile_rows - row0);
    for (int idx = tid; idx < nrows * F4; idx += kRowsThreads) {
        const int  lr = idx / F4, c4 = idx - lr * F4, r = row0 + lr, g = r / a.R, t = r - g * a.R;
        const long id = (((long)b * a.H + hk * a.groups + g) * a.R + t) * splits + split;
        f32x4      val = *reinterpret_cast<const f32x4*>(rec + lr * REC + 4 * c4);
        if (c4 == 0) val[2] = 0.f, val[3] = 0.f;   // the record's pad
        *reinterpret_cast<f32x4*>(a.ws + id * REC + 4 * c4) = val;
    }
}

// The `ns` records of a (batch row, head, query row) into its fp16 output: weights exp2(m_i - max m), one division.  A thread owns
// four channels of one row; a row whose every l is 0 (nothing to attend) gives zeros.  The records' order is the chunks': deterministic.
template <int D>
__global__ __launch_bounds__(256) void attn_rows_merge_kernel(const float* __restrict__ ws, f16* __restrict__ out, long rows, int ns, int R,
                                                              int H, long o_sb, long o_st, long o_sh)
{
    constexpr int TPR = D / 4, REC = D + kRecPad;
    const long    gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long    row = gid / TPR;
    const int     ch  = 4 * (int)(gid % TPR);
    if (row >= rows) return;
    const float* rp = ws + row * ns * REC;
    float        m  = -INFINITY;
    for (int i = 0; i < ns; ++i) m = fmaxf(m, rp[(long)i * REC]);
    const float m_use = m > -INFINITY ? m : 0.f;
    f32x4       acc   = {0.f, 0.f, 0.f, 0.f};
    float       l     = 0.f;
    for (int i = 0; i < ns; ++i) {
        const float w  = __builtin_amdgcn_exp2f(rp[(long)i * REC] - m_use);   // exp2(-inf) = 0: an empty chunk
        const f32x4 oi = *reinterpret_cast<const f32x4*>(rp + (long)i * REC + kRecPad + ch);
        l += w * rp[(long)i * REC + 1];
        acc += w * oi;
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;
    const int   t = (int)(row % R), h = (int)(row / R % H);
    const long  b = row / R / H;
    const f16x2 lo = {(f16)(acc[0] * inv), (f16)(acc[1] * inv)}, hh = {(f16)(acc[2] * inv), (f16)(acc[3] * inv)};
    *reinterpret_cast<u32x2*>(out + b * o_sb + (long)t * o_st + h * o_sh + ch) = u32x2{as_u32(lo), as_u32(hh)};
}

int rows_tile_groups(int H, int Hkv, int R) { return (H / Hkv * R + 16 * kRowsMaxSub - 1) / (16 * kRowsMaxSub); }

template <int D, bool KV8>
int launch_rows_d(const RowsKernArgs<KV8>& a, f16* out, int B, int Hkv, int splits, const long* st, hipStream_t stream)
{
    const dim3 grid((unsigned)splits, (unsigned)(Hkv * a.ntg), (unsigned)B), block(kRowsThreads);
    const int  nsub = a.ntg > 1 ? kRowsMaxSub : (a.groups * a.R + 15) / 16;
    switch (nsub) {
    case 1: launch_kernel(attn_rows_partial_kernel<D, 1, KV8>, grid, block, 0, stream, a); break;
    case 2: launch_kernel(attn_rows_partial_kernel<D, 2, KV8>, grid, block, 0, stream, a); break;
    case 3: launch_kernel(attn_rows_partial_kernel<D, 3, KV8>, grid, block, 0, stream, a); break;
    default: launch_kernel(attn_rows_partial_kernel<D, 4, KV8>, grid, block, 0, stream, a); break;
    }
    EETQ_TRY_HIP(hipGetLastError());
    const long rows = (long)B * a.H * a.R, threads = rows * (D / 4);
    launch_kernel(attn_rows_merge_kernel<D>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, (const float*)a.ws, out, rows,
                  splits, a.R, a.H, st[9], st[10], st[11]);
    return check_hip(hipGetLastError(), "attn_rows kernels launch");
}

}  // namespace

int decode_attention_rows_max_splits() { return kRowsMaxSplits; }

size_t decode_attention_rows_workspace_floats(int B, int H, int R, int D, int splits)
{
    if (B <= 0 || H <= 0 || R <= 0 || D <= 0 || splits <= 0) return 0;
    return (size_t)B * H * R * splits * (D + kRecPad);
}

// The chunk count the two launches are tuned for, from the measured table (profiles/attn_rows.txt):
//   * no more chunks than fill the chip ONCE: the workgroups resident at a time are two per compute unit with one sub-tile and one
//     with more (kernel-resource-usage: 254 and up to 478 registers), and in every row of the table the best count kept the grid
//     within that (40 heads, batch 1: 12 chunks = 480 workgroups 29.9 us behind 4 096 rows, 16 chunks 41.4);
//   * up to 8 chunks a chunk may be as short as 4 blocks (one trip of the four waves), beyond that it keeps 8 (two trips): a shorter
//     chunk's record and its share of the merge cost more than the rows it takes off its neighbours (32 / 8 heads, batch 1, behind
//     1 024 rows: 8 chunks 14.6 us, 4 chunks 15.8, 16 chunks 16.1; behind 4 096: 16 chunks 24.2, 32 chunks 26.0);
//   * never more than 32: the merge walks a row's records one after the other (behind 16 384 rows, 32 / 8 heads: 32 chunks 40.4 us,
//     64 chunks 50.6).  eetq_decode_attention_rows_max_splits() stays 64 for callers that force a count.
int decode_attention_rows_splits(int B, int H, int Hkv, int R, int max_keys)
{
    if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || R <= 0 || max_keys <= 0) return 1;
    const long ntg = rows_tile_groups(H, Hkv, R), wgs = (long)B * Hkv * ntg, cus = device_cu_count();
    const long resident = (long)H / Hkv * R <= 16 ? 2 : 1;   // workgroups per compute unit
    const long blocks = ((long)max_keys + kRowsBlk - 1) / kRowsBlk;
    const long by_chip = resident * cus / wgs, by_len = max(blocks / 8, min(8L, blocks / 4));
    return (int)max(1L, min(32L, min(by_chip, by_len)));
}

namespace {

// what both entries require of the call's shape, before any pointer is followed
int check_rows_shape(int R, int max_keys, int splits, int B, int H, int Hkv, int D, const float* ws)
{
    EETQ_REQUIRE(R >= 1 && R <= kRowsMaxR, "rows must lie in 1 .. 16");
    EETQ_REQUIRE(max_keys > 0, "max_keys must be positive");
    EETQ_REQUIRE(splits >= 1 && splits <= kRowsMaxSplits, "splits must lie in 1 .. 64");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0, "invalid attention shape");
    if (D != 128 && D != 64) return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] few-row attention supports head_dim 64 and 128");
    EETQ_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "the workspace is always needed (two launches) and must be 16-byte aligned");
    return EETQ_OK;
}

// the checked call's arguments into the kernels' block, and the two launches
template <bool KV8>
int launch_rows_checked(RowsKernArgs<KV8>& a, const f16* q, const f16* k, const f16* v, f16* out, float* ws, int B, int H, int Hkv, int R,
                        int max_keys, int D, const int64_t* kv_len, int kv_len_bias, int splits, float scaling, const long* st,
                        hipStream_t stream)
{
    a.q = q, a.k = k, a.v = v, a.ws = ws;
    a.q_sb = st[0], a.q_st = st[1], a.q_sh = st[2], a.k_sb = st[3], a.k_sh = st[4], a.k_ss = st[5];
    a.v_sb = st[6], a.v_sh = st[7], a.v_ss = st[8];
    a.kv_len = kv_len, a.kv_len_bias = kv_len_bias, a.max_keys = max_keys, a.R = R, a.H = H, a.groups = H / Hkv;
    a.ntg = rows_tile_groups(H, Hkv, R);
    a.c = scaling * 1.4426950408889634f;
    EETQ_REQUIRE((long)Hkv * a.ntg <= 65535 && B <= 65535, "too many workgroups");
    EETQ_REQUIRE(((long)B * H * R * (D / 4) + 255) / 256 < (1L << 31), "too many workgroups");
    if (D == 128) return launch_rows_d<128, KV8>(a, out, B, Hkv, splits, st, stream);
    return launch_rows_d<64, KV8>(a, out, B, Hkv, splits, st, stream);
}

}  // namespace

// strides (elements): {q_b, q_row, q_head, k_b, k_head, k_row, v_b, v_head, v_row, out_b, out_row, out_head}
int launch_decode_attention_rows(const f16* q, const f16* k, const f16* v, f16* out, float* ws, int B, int H, int Hkv, int R, int max_keys,
                                 int D, const int64_t* kv_len, int kv_len_bias, int splits, float scaling, const long* st,
                                 hipStream_t stream)
{
    EETQ_REQUIRE(q && k && v && out && st, "null pointer");
    const int rcs = check_rows_shape(R, max_keys, splits, B, H, Hkv, D, ws);
    if (rcs != EETQ_OK) return rcs;
    const int rc = check_attn_layout(q, k, v, out, max_keys, st);
    if (rc != EETQ_OK) return rc;
    // (its own: the row offsets here are unsigned, and kNoRow must lie beyond every row)
    EETQ_REQUIRE(st[5] > 0 && st[8] > 0, "one head's cache rows must span less than 2 GiB");
    RowsArgs a;
    return launch_rows_checked<false>(a, q, k, v, out, ws, B, H, Hkv, R, max_keys, D, kv_len, kv_len_bias, splits, scaling, st, stream);
}

// launch_decode_attention_rows over an int8 cache (kv_i8.hpp): st as there with the k / v entries in BYTES, sst {batch, head, row} of
// the scale pairs in fp16 elements
int launch_decode_attention_rows_i8kv(const f16* q, const int8_t* k, const int8_t* v, const f16* scales, f16* out, float* ws, int B, int H,
                                      int Hkv, int R, int max_keys, int D, const int64_t* kv_len, int kv_len_bias, int splits,
                                      float scaling, const long* st, const long* sst, hipStream_t stream)
{
    EETQ_REQUIRE(q && k && v && scales && out && st && sst, "null pointer");
    const int rc = check_rows_shape(R, max_keys, splits, B, H, Hkv, D, ws);
    if (rc != EETQ_OK) return rc;
    for (int i = 0; i < 3; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q strides must be multiples of 8 elements (16-byte loads)");
    for (int i = 9; i < 12; ++i) EETQ_REQUIRE(st[i] % 4 == 0, "out strides must be multiples of 4 elements");
    EETQ_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)out % 8 == 0, "q must be 16-byte aligned, out 8-byte");
    const int rc8 = check_i8_cache(k, v, scales, max_keys, st + 3, sst);
    if (rc8 != EETQ_OK) return rc8;
    // (the descriptors end at keys * row stride: a row's last chunk must lie inside its own stride)
    EETQ_REQUIRE(st[5] >= D && st[8] >= D, "an int8 cache row stride must hold head_dim bytes");
    RowsArgs8 a;
    a.scales = scales, a.s_sb = sst[0], a.s_sh = sst[1], a.s_ss = sst[2];
    return launch_rows_checked<true>(a, q, reinterpret_cast<const f16*>(k), reinterpret_cast<const f16*>(v), out, ws, B, H, Hkv, R,
                                     max_keys, D, kv_len, kv_len_bias, splits, scaling, st, stream);
}

}  // namespace eetq
