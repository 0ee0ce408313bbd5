// Causal attention over a prompt ("prefill"), fp16 in / fp16 out, fp32 scores, softmax state and accumulation, on MFMA.
//
// No counterpart in the reference's csrc: its EETLlamaAttention hands the attention product to flash-attn
// (python/eetq/modules/llama_modules.py:131-143).  The library kernel torch offers here runs a 1 024-token prompt of 40 heads x 128
// at 76 us per layer (0.14 PFLOP/s of causal work); this is the flash form written for this path: the rotated query rows of the
// fused QKV projection (strided [batch][token][head][D]) against the rows a static KV cache has just been given
// ([batch][kv head][row][D], rows 0 .. keys - 1), query t attending rows <= t + causal_offset.
//
// Workgroup = 4 waves = 128 query rows of one (batch row, head), 32 rows per wave; keys in blocks of 64.
//   S^T = K Q^T   (v_mfma_f32_32x32x16_f16, K rows as the A operand, the wave's Q rows as B: a lane owns ONE query column and 32 of
//                  the block's 64 keys, its partner lane ^ 32 the others -- the row maximum and sum are 31 local operations and one
//                  lane swap; the probabilities, rounded to fp16, ARE the B operand of the next product, no data movement)
//   O^T += V^T P^T (V^T rows = channels as the A operand: V is transposed on its way into LDS -- a thread holds one 16-byte chunk of four
//                  consecutive rows and stores four keys of one channel at a time into a [D][64 keys] image with a 136-byte pitch --
//                  so that a lane's 8 k-slots are two 8-byte reads; the k-slot <-> key assignment
//                  follows what the S^T accumulator layout hands out: slots 0..3 = keys base + 4 hi + j, 4..7 = base + 8 + 4 hi + j)
// K rows sit in LDS as 256-byte rows with their 16-byte chunks XOR-swizzled by (row & 15) (conflict-free 16-byte fragment reads).
// Two LDS buffers, one barrier per block: block j + 1 goes from registers into the free buffer at the top of block j, block j + 2 is
// fetched then and has a whole block of arithmetic to land.  (Issuing block j + 1's score product between block j's softmax and its
// second product -- two barriers per block -- measured the same: the waves of the two resident workgroups run their phases in step.)  Two workgroups per CU (<= 256 registers: everything in the
// architectural file, no accumulator copies).    Blocks beyond a wave's last query row are skipped by that wave; heavy query blocks are
// dispatched first (1-D grid ordered by weight).
// The device-length and split forms also run over an int8 KV cache (KV8, kv_i8.hpp), with a per-row first key (PAD) and with a
// sliding window (WIN), the latter also over a ring cache (RING): see the comment above the kernel.
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "kv_i8.hpp"

namespace eetq {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kPfThreads = 256, kPfBM = 128, kPfBN = 64;

struct PrefillArgs {
    const f16* q;
    const f16* k;
    const f16* v;
    f16*       out;
    long       q_sb, q_st, q_sh, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss, o_sb, o_st, o_sh;
    int        Tq, Tk, koff, groups, H, B, nqb;
    float      c;   // scaling * log2(e)
};

// The device-length and split-KV forms (kPfDev, kPfSplit) take the cache's length from a device counter and / or hand the key blocks
// of a workgroup to `ns` workgroups.  Their arguments ride behind the host form's, which keeps its own kernarg block.
struct PrefillDevArgs : PrefillArgs {
    const int64_t* kv_len;   // DEVICE scalar or nullptr (then Tk is the host's); Tk = clamp(*kv_len + kv_len_bias, 0, Tk), koff = Tk - Tq
    float*         ws;       // split form: per (b, h, query row, split) D unnormalised fp32 accumulators, then the (m, l) pairs
    int            kv_len_bias, ns;
};
constexpr int kPfHost = 0, kPfDev = 1, kPfSplit = 2;
constexpr int kPfMaxSplits = 16;
// The int8-row form (KV8; kv_i8.hpp): k and v point at int8 rows, their strides are in BYTES, and the row's scale
// pair (k scale, v scale) lies in `scales`.  Behind the fp16 forms' arguments, which keep their kernarg blocks.
struct PrefillDevArgs8 : PrefillDevArgs {
    const f16* scales;
    long       s_sb, s_sh, s_ss;   // fp16 elements between batch rows, kv heads, rows of the scale tensor
};
// The per-row first key (PAD): batch row b's cache rows below kv_start[b] are padding.  Behind the device-length
// arguments, which keep their kernarg block.
struct PrefillPadArgs : PrefillDevArgs {
    const int64_t* kv_start;   // DEVICE [batch]
};
// The sliding window (WIN): a query at cache row p attends rows max(0, p - window + 1) .. p.  Behind the device-length
// arguments, which keep their kernarg block.
struct PrefillWinArgs : PrefillDevArgs {
    int window;   // >= 1, a host constant of the model
};
// The ring cache (RING, on top of WIN): k and v are rings of 64 * ring_blocks rows, logical row r at physical row
// r mod (64 * ring_blocks).  Behind the windowed arguments, which keep their kernarg block.
struct PrefillRingArgs : PrefillWinArgs {
    int ring_blocks;   // R / 64 >= 1
};
template <int MODE, bool KV8, bool PAD = false, bool WIN = false, bool RING = false>
using PrefillKernArgs = std::conditional_t<
    RING, PrefillRingArgs,
    std::conditional_t<WIN, PrefillWinArgs,
                       std::conditional_t<PAD, PrefillPadArgs,
                                          std::conditional_t<KV8, PrefillDevArgs8,
                                                             std::conditional_t<MODE == kPfHost, PrefillArgs, PrefillDevArgs>>>>>;

// MODE kPfHost: keys and causal offset from the host (the fresh prompt's path, unchanged).  kPfDev: every workgroup reads the length
// at entry -- one scalar load -- and forms Tk and koff itself; kend, nblk, the descriptors' range, `active` and `edge` follow, the
// grid depends on Tq alone.  kPfSplit: workgroup id / ns is the (query block, head, batch row) of the other forms, id % ns its
// share [i nblk / ns, (i + 1) nblk / ns) of that workgroup's key blocks; it leaves (o, m, l) per row in the workspace, an empty
// share or a row with nothing to attend as (zeros, -inf, 0), and prefill_merge_kernel divides.
//
// KV8 (kPfDev and kPfSplit only): the same tiles over an int8 cache.  What changes is fetch and stage:
//   * a thread's share of a row is 8 bytes -- the same (rows p4 .. p4 + NLD - 1, chunk c16) ownership with 8-byte loads -- and the
//     rows' scale dwords come through a third descriptor that ends at the valid length as well: a row at or beyond Tk reads as
//     bytes 0, scale 0;
//   * K bytes enter the swizzled image as exact fp16 integers (kv8_unpack8) and the K scale is folded into the score in fp32 behind
//     the product, before the mask and the maximum: (ks * scaling) * (q . k8), the decode entries' contract.  The tile's 64 K scales
//     sit in LDS as fp32, per buffer;
//   * a V row enters the transposed image as fp16(vs * v8): one packed fp16 multiply of the exact integer by the row's scale, a single
//     rounding of the exact product, denormals kept.  THE ONE DIFFERENCE from the decode entries, which fold vs into the probability
//     in fp32: here 2^12 p * vs would leave the fp16 range (vs spans 2^-24 .. 516).  A row that holds all the weight still comes out
//     as fp16(vs * v8) bit for bit.
//
// PAD (kPfDev and kPfSplit, fp16 rows): batch row b starts at cache row s = clamp(kv_start[b], 0, Tk).  Its first p = clamp(s - koff, 0, Tq)
// queries are padding and come out as zeros (zero records in the split form); then the row is MOVED: q and out by p tokens, k and v by
// s rows, Tq -= p, Tk -= s, koff = Tk - Tq, and the unchanged code below runs in the row's own frame -- query blocks, key blocks and
// split shares counted from its first real token, the descriptors starting there: the bits of the plain form called on that row
// alone, and no row below s is read.  Workgroups whose query block lies beyond the row's real queries leave.
//
// WIN (kPfDev and kPfSplit, fp16 rows): query row t (cache row t + koff) attends keys in (t + koff - W, t + koff].  The key-block grid
// stays absolute (blocks of 64 from row 0); a workgroup starts at its first needed block jlo = max(0, q0 + koff - W + 1) / 64 -- loop,
// prologue and, in the split form, the shares [jlo + i n / ns, jlo + (i + 1) n / ns) of its n = nblk - jlo blocks --, a wave skips the
// blocks that end below its first row's window, and the mask has a lower edge.  A row whose first blocks are fully masked keeps
// m_run = -inf and every p = 0 until its window begins.  W >= keys: jlo = 0 and no lower edge is ever taken -- the bits of the
// plain form; so are, in any launch, the rows with t + koff < W (their workgroup starts at block 0 and their wave skips nothing the
// plain form attends).  No row below 64 (max(0, koff - W + 1) / 64) is read by the launch; rows of a lower-edge block below a row's
// window are read and enter the value product with probability 0 (they must be finite).
//
// RING (with WIN): Tk, koff, the key-block grid, jlo, the shares, the wave skip and both mask edges stay in LOGICAL rows and may exceed
// the ring; only the address of a key block changes.  The descriptors cover the R = 64 ring_blocks rows of the ring, and block j is
// fetched from physical block j mod ring_blocks (R % 64 == 0: a block never straddles the ring's end): blocks are fetched in order,
// so the physical block is a counter that starts at j0 mod ring_blocks -- the launch's one division -- and wraps with one scalar
// compare, in front of the tile offset that rides in the loads' scalar operand.  What the descriptor clipped in the static forms --
// the rows of the upper-edge block at and beyond Tk -- are rows of the ring here, stale or never written: they are masked exactly
// as the rows below a window are and enter the value product with probability 0, so every ring row must be finite.  The host keeps
// R >= W + Tq + 62: no key block the launch reads holds a row the call's own cache write has replaced.
template <int D, int MODE, bool KV8 = false, bool PAD = false, bool WIN = false, bool RING = false>
__global__ __launch_bounds__(kPfThreads, 2) void prefill_attn_kernel(const PrefillKernArgs<MODE, KV8, PAD, WIN, RING> a_in)
{
    static_assert(!RING || WIN, "the ring rides on the window");
    static_assert(!KV8 || MODE != kPfHost, "the int8-row form takes the device-length arguments");
    static_assert(!PAD || (MODE != kPfHost && !KV8), "the per-row first key rides on the device-length arguments, fp16 rows");
    static_assert(!WIN || (MODE != kPfHost && !KV8 && !PAD), "the window rides on the device-length arguments, fp16 rows, one first key");
    PrefillArgs a = a_in;
    int         wg = (int)blockIdx.x, split = 0;
    if constexpr (MODE != kPfHost) {
        if (a_in.kv_len) {
            const int64_t n = *a_in.kv_len + (int64_t)a_in.kv_len_bias;   // uniform: a scalar load
            a.Tk = (int)max((int64_t)0, min((int64_t)a.Tk, n));
        }
        a.koff = a.Tk - a.Tq;
    }
    if constexpr (MODE == kPfSplit) {
        split = wg % a_in.ns;
        wg /= a_in.ns;
    }
    static_assert(D == 128 || D == 64, "head_dim 128 or 64");
    constexpr int KS = D / 16;            // k-steps of the score product
    constexpr int DT = D / 32;            // 32-channel blocks of the output
    constexpr int VT_PITCH = kPfBN + 4;   // halfs per channel row of the transposed V image (136 bytes)
    constexpr int CH = D / 8;             // 16-byte chunks per K / V row
    constexpr int NLD = kPfBN * CH / kPfThreads;  // 16-byte loads per thread and tile
    // two LDS buffers (2 x 33 KiB): block j is read from buffer j & 1 while block j + 1 -- fetched into registers during block j - 1 -- is
    // written into the other one at the top of block j and block j + 2 is fetched: global loads have a whole block of arithmetic to
    // land, one barrier per block
    __shared__ __attribute__((aligned(16))) f16 k_lds2[2][kPfBN * D];
    __shared__ __attribute__((aligned(16))) f16 vt_lds2[2][D * VT_PITCH];
    __shared__ __attribute__((aligned(16))) float ks_lds2[2][KV8 ? kPfBN : 1];   // KV8: the tile's K scales

    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, ln = lane & 31, hi = lane >> 5;
    // (wave in a scalar register: the per-wave tests below -- block skipped, block on the diagonal -- must be branches, not selects)
    // 1-D grid, heaviest query blocks first: id -> (query block rank, head, batch row).  With H * B a multiple of 8 all query blocks
    // of a head land on one XCD (its K / V rows are shared in that L2), and a CU's second workgroup is a light one
    const int hb = a.H * a.B, qb = a.nqb - 1 - wg / hb, rest = wg % hb;
    const int h = rest % a.H, b = rest / a.H, hk = h / a.groups;
    const int q0 = qb * kPfBM, qrow = q0 + wave * 32 + ln;           // this lane's query row
    int       pad_q = 0;                                              // PAD: the row's pad queries (qrow counts from the first real one)
    const int Tq_all = a.Tq;
    if constexpr (PAD) {
        const int s = (int)max((int64_t)0, min((int64_t)a.Tk, a_in.kv_start[b]));   // uniform: a scalar load
        pad_q = max(0, min(a.Tq, s - a.koff));
        // the pad queries of this workgroup's 128 rows (counted from the row's first token): zeros, in the layout of the stores below
        if (qrow < pad_q) {
            if constexpr (MODE == kPfSplit) {
                const long rec  = (((long)b * a.H + h) * Tq_all + qrow) * a_in.ns + split;
                const long recs = (long)a.B * a.H * Tq_all * a_in.ns;
                float*     wp   = a_in.ws + rec * D + 4 * hi;
#pragma unroll
                for (int i = 0; i < D / 8; ++i) *reinterpret_cast<f32x4*>(wp + 8 * i) = f32x4{0.f, 0.f, 0.f, 0.f};
                if (hi == 0) {
                    a_in.ws[recs * D + 2 * rec]     = -INFINITY;
                    a_in.ws[recs * D + 2 * rec + 1] = 0.f;
                }
            } else {
                f16* op = a.out + b * a.o_sb + (long)qrow * a.o_st + h * a.o_sh + 4 * hi;
#pragma unroll
                for (int i = 0; i < D / 8; ++i) *reinterpret_cast<u32x2*>(op + 8 * i) = u32x2{0u, 0u};
            }
        }
        a.q += (long)pad_q * a.q_st, a.out += (long)pad_q * a.o_st;
        a.k += (long)s * a.k_ss, a.v += (long)s * a.v_ss;
        a.Tq -= pad_q, a.Tk -= s, a.koff = a.Tk - a.Tq;
        if (q0 >= a.Tq) return;   // workgroup-uniform, before any barrier: no real query in this block
    }
    const int qlast_wave = q0 + wave * 32 + 31;                       // the wave's last row
    // keys this workgroup needs: rows <= its last query + koff
    const int kend  = min(a.Tk, q0 + kPfBM + a.koff);
    const int nblk  = kend > 0 ? (kend + kPfBN - 1) / kPfBN : 0;
    // this workgroup's key blocks [j0, j1): all of them, or its share
    int j0 = 0, j1 = nblk;
    int wlo = 0;   // WIN: koff - W + 1; row t's first attended key is t + wlo
    if constexpr (WIN) {
        wlo = a.koff - a_in.window + 1;
        j0  = min(nblk, max(0, q0 + wlo) / kPfBN);   // the first block a row of this workgroup attends
    }
    if constexpr (MODE == kPfSplit) {
        const int jlo = j0, n = nblk - jlo;
        j0 = jlo + (int)((long)split * n / a_in.ns);
        j1 = jlo + (int)((long)(split + 1) * n / a_in.ns);
    }
    // the valid rows of this (batch row, kv head) behind buffer descriptors: rows at and beyond Tk are out of range and read as zeros
    // (KV8: the same three lines with strides in bytes, and the rows' scale dwords behind a third descriptor)
    constexpr unsigned EB = KV8 ? 1u : 2u;   // bytes per unit of the cache strides
    __amdgpu_buffer_rsrc_t krs, vrs, srs;
    if constexpr (KV8) {
        const char* kbase = reinterpret_cast<const char*>(a.k) + b * a.k_sb + hk * a.k_sh;
        const char* vbase = reinterpret_cast<const char*>(a.v) + b * a.v_sb + hk * a.v_sh;
        krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(kbase), 0, (int)((unsigned)a.Tk * (unsigned)a.k_ss), 0x00020000);
        vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(vbase), 0, (int)((unsigned)a.Tk * (unsigned)a.v_ss), 0x00020000);
        srs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(a_in.scales + b * a_in.s_sb + hk * a_in.s_sh), 0,
                                                (int)((unsigned)a.Tk * (unsigned)a_in.s_ss * 2u), 0x00020000);
    } else {
        unsigned rows = (unsigned)a.Tk;
        if constexpr (RING) rows = (unsigned)(a_in.ring_blocks * kPfBN);   // the whole ring
        krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(a.k + b * a.k_sb + hk * a.k_sh), 0,
                                                (int)(rows * (unsigned)a.k_ss * 2u), 0x00020000);
        vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(a.v + b * a.v_sb + hk * a.v_sh), 0,
                                                (int)(rows * (unsigned)a.v_ss * 2u), 0x00020000);
        srs = krs;   // not used
    }

    // ---- the wave's query rows as B fragments: lane (ln, hi) holds channels 16 ks + 8 hi .. + 7 of row ln ----
    f16x8 qf[KS];
    {
        const f16* qp = a.q + b * a.q_sb + (long)min(qrow, a.Tq - 1) * a.q_st + h * a.q_sh + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const f16x8*>(qp + 16 * ks);
    }

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // staging registers: thread t holds 16-byte chunk t % CH of the NLD consecutive rows NLD (t / CH) .. of a tile (four rows at D = 128,
    // two at D = 64) -- so that the transposed V image is written as 8- / 4-byte pieces (NLD keys of one channel: 8 LDS writes per
    // thread and tile; 2-byte writes, 64 of them, kept the LDS pipe busy for ~4 000 cycles per tile and workgroup)
    static_assert((NLD == 4 && CH == 16) || (NLD == 2 && CH == 8), "rows per thread");
    // KV8: the chunk is the row's 8 bytes of the same 8 channels, and every thread also holds its rows' scale dwords (the CH threads
    // of a row read the same address); the rows' V scales are needed by all of them, the K scales go to LDS from chunk 0's thread
    using StageReg = std::conditional_t<KV8, u32x2, u32x4>;
    StageReg  kreg[NLD], vreg[NLD];
    u32       sreg[KV8 ? NLD : 1];
    const int c16 = tid % CH, p4 = NLD * (tid / CH);
    const int krow_b = (int)(a.k_ss * EB), vrow_b = (int)(a.v_ss * EB);
    constexpr int CB = KV8 ? 8 : 16;       // bytes of a thread's chunk in the cache
    const int kvo = p4 * krow_b + c16 * CB, vvo = p4 * vrow_b + c16 * CB;  // constant; tile and row offsets ride in the scalar operand
    int srow_b = 0, svo = 0;
    if constexpr (KV8) srow_b = (int)(a_in.s_ss * 2), svo = p4 * srow_b;
    int pj = 0;   // RING: the physical block of the next fetch (fetches go block by block from j0)
    if constexpr (RING) pj = j0 % a_in.ring_blocks;
    auto fetch = [&](int j) {
        if constexpr (RING) {
            j  = pj;
            pj = pj + 1 == a_in.ring_blocks ? 0 : pj + 1;
        }
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            if constexpr (KV8) {
                kreg[r] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(krs, kvo, (j * kPfBN + r) * krow_b, 0));
                vreg[r] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(vrs, vvo, (j * kPfBN + r) * vrow_b, 0));
                sreg[r] = __builtin_amdgcn_raw_buffer_load_b32(srs, svo, (j * kPfBN + r) * srow_b, 0);
            } else {
                kreg[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, kvo, (j * kPfBN + r) * krow_b, 0));
                vreg[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vrs, vvo, (j * kPfBN + r) * vrow_b, 0));
            }
        }
    };
    // KV8: 8 bytes -> the 16-byte chunk the fp16 form holds; K as the exact integers, V as fp16(vs * v8)
    auto chunk8 = [](const u32x2& w) {
        f16x2 h[4];
        kv8_unpack8(w, h);
        return f16x8{h[0][0], h[0][1], h[1][0], h[1][1], h[2][0], h[2][1], h[3][0], h[3][1]};
    };
    auto kchunk = [&](int r) {
        if constexpr (KV8) return __builtin_bit_cast(u32x4, chunk8(kreg[r]));
        else return kreg[r];
    };
    auto vchunk = [&](int r) {
        if constexpr (KV8) {
            f16x2 h[4];
            kv8_unpack8(vreg[r], h);
            const f16   vs  = as_f16x2(sreg[r])[1];
            const f16x2 vs2 = {vs, vs};
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = h[i] * vs2;   // one rounding of the exact product
            return f16x8{h[0][0], h[0][1], h[1][0], h[1][1], h[2][0], h[2][1], h[3][0], h[3][1]};
        } else {
            return __builtin_bit_cast(f16x8, vreg[r]);
        }
    };
    // K rows: 16-byte chunks XOR-swizzled by (row & (CH - 1)).  V^T image: channel row d, key column key ^ (((d >> 5) & 3) << 3): a
    // wave's stores land in different banks.
    auto stage = [&](int buf) {
        f16* kl = k_lds2[buf];
        f16* vl = vt_lds2[buf];
#pragma unroll
        for (int r = 0; r < NLD; ++r) *reinterpret_cast<u32x4*>(kl + (p4 + r) * D + 8 * (c16 ^ ((p4 + r) & (CH - 1)))) = kchunk(r);
        if constexpr (KV8) {
            if (c16 == 0) {
#pragma unroll
                for (int r = 0; r < NLD; ++r) ks_lds2[buf][p4 + r] = (float)as_f16x2(sreg[r])[0];
            }
        }
        f16* vp = vl + 8 * c16 * VT_PITCH + (p4 ^ (((c16 >> 2) & 3) << 3));
        const f16x8 v0 = vchunk(0), v1 = vchunk(1);
        if constexpr (NLD == 4) {
            const f16x8 v2 = vchunk(2), v3 = vchunk(3);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const f16x2 lo = {v0[e], v1[e]}, hh = {v2[e], v3[e]};
                *reinterpret_cast<u32x2*>(vp + e * VT_PITCH) = u32x2{as_u32(lo), as_u32(hh)};
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const f16x2 lo = {v0[e], v1[e]};
                *reinterpret_cast<u32*>(vp + e * VT_PITCH) = as_u32(lo);
            }
        }
    };

    if (j1 > j0) {
        fetch(j0);
        stage(j0 & 1);
        if (j1 > j0 + 1) fetch(j0 + 1);
    }
    __syncthreads();

    for (int j = j0; j < j1; ++j) {
        const int  key0   = j * kPfBN;
        bool       active = key0 <= qlast_wave + a.koff;  // wave-uniform: some row of this wave attends this block
        if constexpr (WIN) active = active && key0 + kPfBN - 1 >= q0 + wave * 32 + wlo;   // ... and it does not end below the wave's window
        if (j + 1 < j1) stage((j + 1) & 1);               // block j + 1: registers -> the buffer block j - 1 was read from
        if (j + 2 < j1) fetch(j + 2);
        const f16* k_lds  = k_lds2[j & 1];
        const f16* vt_lds = vt_lds2[j & 1];
        if (active) {
            // ---- S^T = K Q^T: two 32-key halves (alternating: back-to-back MFMAs on one accumulator wait out each other's latency) ----
            f32x16 s[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    const int   krow = 32 * kb + ln;
                    const f16x8 kf = *reinterpret_cast<const f16x8*>(k_lds + krow * D + 8 * ((2 * ks + hi) ^ (krow & (CH - 1))));
                    s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[kb], 0, 0, 0);
                }
            // KV8: the K scale into the score, in fp32: accumulator values 4 g .. 4 g + 3 are keys 32 kb + 8 g + 4 hi + {0..3}, one
            // 16-byte read (the same address across ln)
            if constexpr (KV8) {
                const float* ksl = ks_lds2[j & 1] + 4 * hi;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 sc = *reinterpret_cast<const f32x4*>(ksl + 32 * kb + 8 * g);
#pragma unroll
                        for (int i = 0; i < 4; ++i) s[kb][4 * g + i] *= sc[i];
                    }
            }
            // ---- mask (only where the block touches the wave's diagonal or the end of the keys: a wave-uniform branch), running maximum
            // (scaled domain) ----
            bool edge = key0 + kPfBN - 1 > q0 + wave * 32 + a.koff || key0 + kPfBN > a.Tk;
            // the lower edge: the block begins below the window of the wave's last real row
            if constexpr (WIN) edge = edge || key0 < min(qlast_wave, a.Tq - 1) + wlo;
            float mloc = -INFINITY;
            if (edge) {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int  key   = key0 + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        bool       valid = key < a.Tk && key <= qrow + a.koff;
                        if constexpr (WIN) valid = valid && key >= qrow + wlo;
                        float      t     = valid ? s[kb][r] : -INFINITY;
                        asm volatile("" : "+v"(t));  // pins the select inside the branch (else: 170 select instructions on EVERY block)
                        s[kb][r] = t;
                    }
            }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, s[kb][r]);
            mloc = fmaf(fmaxf(mloc, __shfl_xor(mloc, 32, 64)), a.c, -kAttnPShift);   // (c > 0); the maxima are kept 12 below: p as 2^12 p
            const float m_new = fmaxf(m_run, mloc);
            const float m_use = m_new > -INFINITY ? m_new : 0.f;             // a row with nothing to attend yet: every p = 0
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);       // exp2(-inf) = 0 for the first block
            float       psum  = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[kb][r] = __builtin_amdgcn_exp2f(fmaf(s[kb][r], a.c, -m_use));
                    psum += s[kb][r];
                }
            psum += __shfl_xor(psum, 32, 64);
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
            // ---- O^T += V^T P^T: per 32-key half two 16-key steps; the lane's own accumulator values are its B operand ----
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    f16x8 pf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[e] = (f16)s[kb][8 * st + e];
                    const int kcol = 32 * kb + 16 * st + 4 * hi;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        const f16*  vrow = vt_lds + (32 * dt + ln) * VT_PITCH;
                        const u32x2 v0 = *reinterpret_cast<const u32x2*>(vrow + (kcol ^ (dt << 3)));
                        const u32x2 v1 = *reinterpret_cast<const u32x2*>(vrow + ((kcol + 8) ^ (dt << 3)));
                        const f16x8 vf = __builtin_bit_cast(f16x8, u32x4{v0.x, v0.y, v1.x, v1.y});
                        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, o[dt], 0, 0, 0);
                    }
                }
        }
        __syncthreads();       // block j has been read by every wave; block j + 1 is in the other buffer
    }

    // ---- split form: the row's record, unnormalised (the 2^12 carry is in o and l alike and leaves in the merge's division) ----
    if constexpr (MODE == kPfSplit) {
        if (qrow < a.Tq) {
            const long rec  = (((long)b * a.H + h) * Tq_all + qrow + pad_q) * a_in.ns + split;
            const long recs = (long)a.B * a.H * Tq_all * a_in.ns;
            float*     wp   = a_in.ws + rec * D + 4 * hi;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<f32x4*>(wp + 32 * dt + 8 * g) =
                        f32x4{o[dt][4 * g + 0], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]};
            if (hi == 0) {   // both halves of a lane pair hold the row's m and l
                a_in.ws[recs * D + 2 * rec]     = m_run;
                a_in.ws[recs * D + 2 * rec + 1] = l_run;
            }
        }
        return;
    }
    // ---- normalise and store: lane (ln, hi) holds row `qrow`, channels 32 dt + 8 g + 4 hi .. + 3 ----
    if (qrow < a.Tq) {
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        f16*        op  = a.out + b * a.o_sb + (long)qrow * a.o_st + h * a.o_sh + 4 * hi;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f16x2 lo = {(f16)(o[dt][4 * g + 0] * inv), (f16)(o[dt][4 * g + 1] * inv)};
                const f16x2 hh = {(f16)(o[dt][4 * g + 2] * inv), (f16)(o[dt][4 * g + 3] * inv)};
                *reinterpret_cast<u32x2*>(op + 32 * dt + 8 * g) = u32x2{as_u32(lo), as_u32(hh)};
            }
    }
}

// The `ns` records of a query row into its fp16 output: weights exp2(m_i - max m), one division.  A thread owns four channels of
// one (b, h, row); a row whose every l is 0 (nothing to attend) gives zeros.  The records' order is the splits': deterministic.
template <int D>
__global__ __launch_bounds__(256) void prefill_merge_kernel(const float* __restrict__ ws, f16* __restrict__ out, long rows, int ns, int Tq,
                                                            int H, long o_sb, long o_st, long o_sh)
{
    constexpr int TPR = D / 4;   // threads per row
    const long    gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long    row = gid / TPR;
    const int     ch  = 4 * (int)(gid % TPR);
    if (row >= rows) return;
    const float* ml = ws + rows * ns * D + 2 * row * ns;
    float        m  = -INFINITY;
    for (int i = 0; i < ns; ++i) m = fmaxf(m, ml[2 * i]);
    const float m_use = m > -INFINITY ? m : 0.f;
    f32x4       acc   = {0.f, 0.f, 0.f, 0.f};
    float       l     = 0.f;
    for (int i = 0; i < ns; ++i) {
        const float w = __builtin_amdgcn_exp2f(ml[2 * i] - m_use);   // exp2(-inf) = 0: an empty share
        const f32x4 o = *reinterpret_cast<const f32x4*>(ws + (row * ns + i) * D + ch);
        l += w * ml[2 * i + 1];
        acc += w * o;
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;
    const int   t = (int)(row % Tq), h = (int)(row / Tq % H);
    const long  b = row / Tq / H;
    const f16x2 lo = {(f16)(acc[0] * inv), (f16)(acc[1] * inv)}, hh = {(f16)(acc[2] * inv), (f16)(acc[3] * inv)};
    *reinterpret_cast<u32x2*>(out + b * o_sb + (long)t * o_st + h * o_sh + ch) = u32x2{as_u32(lo), as_u32(hh)};
}

int check_prefill_common(const f16* q, const f16* k, const f16* v, f16* out, int B, int H, int Hkv, int Tq, int Tk, int D, const long* st)
{
    EETQ_REQUIRE(q && k && v && out && st, "null pointer");
    EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && Tq > 0 && Tk > 0, "invalid attention shape");
    if (!prefill_attention_supports(D)) return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] prompt attention supports head_dim 64 and 128");
    const int rc = check_attn_layout(q, k, v, out, Tk, st);
    if (rc != EETQ_OK) return rc;
    EETQ_REQUIRE((long)((Tq + kPfBM - 1) / kPfBM) * H * B < (1L << 31), "too many workgroups");
    return EETQ_OK;
}

void fill_prefill_args(PrefillArgs& a, const f16* q, const f16* k, const f16* v, f16* out, int B, int H, int Hkv, int Tq, int Tk,
                       int causal_offset, float scaling, const long* st)
{
    a.q = q, a.k = k, a.v = v, a.out = out;
    a.q_sb = st[0], a.q_st = st[1], a.q_sh = st[2], a.k_sb = st[3], a.k_sh = st[4], a.k_ss = st[5];
    a.v_sb = st[6], a.v_sh = st[7], a.v_ss = st[8], a.o_sb = st[9], a.o_st = st[10], a.o_sh = st[11];
    a.Tq = Tq, a.Tk = Tk, a.koff = causal_offset, a.groups = H / Hkv;
    a.c = scaling * 1.4426950408889634f;
    a.H = H, a.B = B, a.nqb = (Tq + kPfBM - 1) / kPfBM;
}

}  // namespace

bool prefill_attention_supports(int D) { return D == 128 || D == 64; }

// what the 16-byte loads, the 8-byte stores and the 32-bit offsets behind the cache descriptors ask of the layout
int check_attn_layout(const f16* q, const f16* k, const f16* v, const f16* out, int keys, const long* st)
{
    for (int i = 0; i < 12; ++i) EETQ_REQUIRE(st[i] % 4 == 0, "strides must be multiples of 4 elements");
    for (int i = 0; i < 9; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q / k / v strides must be multiples of 8 elements (16-byte loads)");
    EETQ_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) % 16 == 0 && (uintptr_t)out % 8 == 0, "q, k, v must be 16-byte aligned, out 8-byte");
    EETQ_REQUIRE((long)keys * st[5] * 2 < (1L << 31) && (long)keys * st[8] * 2 < (1L << 31), "one head's cache rows must span less than 2 GiB");
    return EETQ_OK;
}

// strides (elements): {q_b, q_token, q_head, k_b, k_head, k_row, v_b, v_head, v_row, out_b, out_token, out_head}
int launch_prefill_attention(const f16* q, const f16* k, const f16* v, f16* out, int B, int H, int Hkv, int Tq, int Tk, int D,
                             int causal_offset, float scaling, const long* st, hipStream_t stream)
{
    const int rc = check_prefill_common(q, k, v, out, B, H, Hkv, Tq, Tk, D, st);
    if (rc != EETQ_OK) return rc;
    PrefillArgs a;
    fill_prefill_args(a, q, k, v, out, B, H, Hkv, Tq, Tk, causal_offset, scaling, st);
    if (D == 128)
        launch_kernel(prefill_attn_kernel<128, kPfHost>, dim3((unsigned)(a.nqb * H * B)), dim3(kPfThreads), 0, stream, a);
    else
        launch_kernel(prefill_attn_kernel<64, kPfHost>, dim3((unsigned)(a.nqb * H * B)), dim3(kPfThreads), 0, stream, a);
    return check_hip(hipGetLastError(), "prefill_attn_kernel launch");
}

int prefill_attention_max_splits() { return kPfMaxSplits; }

size_t prefill_attention_workspace_floats(int B, int H, int Tq, int D, int splits)
{
    if (B <= 0 || H <= 0 || Tq <= 0 || D <= 0 || splits <= 1) return 0;
    return (size_t)B * H * Tq * splits * (D + 2);
}

// The count the split form is worth, from the measured table (profiles/prefill_attn_append.txt): shares are doubled while
// the grid stays within 1.25 workgroups per compute unit and every share keeps enough key blocks to pay for its record and the merge
// launch -- 4 blocks (256 keys) while the grid covers at most half the compute units, 8 up to all of them, 16 beyond.  1 wherever the
// query blocks alone fill the chip.  Never more shares than key blocks.
int prefill_attention_splits(int B, int H, int Tq, int max_keys)
{
    if (B <= 0 || H <= 0 || Tq <= 0 || max_keys <= 0) return 1;
    const long wgs = (long)((Tq + kPfBM - 1) / kPfBM) * H * B, cus = device_cu_count();
    const long blocks = ((long)max_keys + kPfBN - 1) / kPfBN;
    long       ns = 1;
    for (long n = 2; n <= kPfMaxSplits; n *= 2) {
        const long grid = n * wgs;
        if (4 * grid > 5 * cus) break;
        const long min_blocks = 2 * grid <= cus ? 4 : grid <= cus ? 8 : 16;
        if (blocks / n < min_blocks) break;
        ns = n;
    }
    return (int)ns;
}

namespace {

// The one launch path of the device forms (plain, per-row first key, int8 rows).  `a` arrives with the form's own fields set
// (kv_start; the scales), `front` runs the form's own argument checks -- every form has them between the two requirements on top
// and the workspace's --, what1 / whatn name the form when a launch fails.  k and v: the int8 form's rows as they go into the struct.
template <bool KV8, bool PAD, bool WIN = false, bool RING = false, class Front>
int launch_prefill_forms(PrefillKernArgs<kPfDev, KV8, PAD, WIN, RING>& a, Front front, const f16* q, const f16* k, const f16* v, f16* out, float* ws,
                         int B, int H, int Hkv, int Tq, int max_keys, int D, const int64_t* kv_len, int kv_len_bias, int splits,
                         float scaling, const long* st, hipStream_t stream, const char* what1, const char* whatn)
{
    EETQ_REQUIRE(max_keys > 0, "max_keys must be positive");
    EETQ_REQUIRE(splits >= 1 && splits <= kPfMaxSplits, "splits must lie in 1 .. 16");
    const int rc = front();
    if (rc != EETQ_OK) return rc;
    EETQ_REQUIRE(splits == 1 || (ws && (uintptr_t)ws % 16 == 0), "the split form needs a 16-byte aligned workspace");
    fill_prefill_args(a, q, k, v, out, B, H, Hkv, Tq, max_keys, max_keys - Tq, scaling, st);
    a.kv_len = kv_len, a.ws = ws, a.kv_len_bias = kv_len_bias, a.ns = splits;
    const long wgs = (long)a.nqb * H * B * splits;
    EETQ_REQUIRE(wgs < (1L << 31), "too many workgroups");
    const dim3 grid((unsigned)wgs), block(kPfThreads);
    if (splits == 1) {
        if (D == 128)
            launch_kernel(prefill_attn_kernel<128, kPfDev, KV8, PAD, WIN, RING>, grid, block, 0, stream, a);
        else
            launch_kernel(prefill_attn_kernel<64, kPfDev, KV8, PAD, WIN, RING>, grid, block, 0, stream, a);
        return check_hip(hipGetLastError(), what1);
    }
    const long rows = (long)B * H * Tq, threads = rows * (D / 4);
    EETQ_REQUIRE((threads + 255) / 256 < (1L << 31), "too many workgroups");
    const dim3 mgrid((unsigned)((threads + 255) / 256));
    if (D == 128) {
        launch_kernel(prefill_attn_kernel<128, kPfSplit, KV8, PAD, WIN, RING>, grid, block, 0, stream, a);
        launch_kernel(prefill_merge_kernel<128>, mgrid, dim3(256), 0, stream, (const float*)ws, out, rows, splits, Tq, H, st[9], st[10], st[11]);
    } else {
        launch_kernel(prefill_attn_kernel<64, kPfSplit, KV8, PAD, WIN, RING>, grid, block, 0, stream, a);
        launch_kernel(prefill_merge_kernel<64>, mgrid, dim3(256), 0, stream, (const float*)ws, out, rows, splits, Tq, H, st[9], st[10], st[11]);
    }
    return check_hip(hipGetLastError(), whatn);
}

}  // namespace

// Device-length and split-KV launches: keys <= max_keys from *kv_len + kv_len_bias (kv_len nullptr: max_keys itself), causal offset
// keys - Tq.  splits > 1: two plain launches, the shares into `ws` (prefill_attention_workspace_floats), then the merge.
int launch_prefill_attention_dev(const f16* q, const f16* k, const f16* v, f16* out, float* ws, int B, int H, int Hkv, int Tq, int max_keys,
                                 int D, const int64_t* kv_len, int kv_len_bias, int splits, float scaling, const long* st, hipStream_t stream)
{
    // nothing for the device to decide: the host form, whose checks are the ones below (a max_keys <= 0 is reported here)
    if (max_keys > 0 && splits == 1 && !kv_len)
        return launch_prefill_attention(q, k, v, out, B, H, Hkv, Tq, max_keys, D, max_keys - Tq, scaling, st, stream);
    PrefillDevArgs a;
    return launch_prefill_forms<false, false>(
        a, [&] { return check_prefill_common(q, k, v, out, B, H, Hkv, Tq, max_keys, D, st); }, q, k, v, out, ws, B, H, Hkv, Tq, max_keys, D,
        kv_len, kv_len_bias, splits, scaling, st, stream, "prefill_attn_kernel (device length) launch", "prefill_attn_kernel (split) launch");
}

// launch_prefill_attention_dev with a per-row first key: cache rows below kv_start[b] (DEVICE [B]) of batch row b are padding (the PAD
// form above).  Always the device-length kernel (kv_len nullptr: max_keys keys), or the split form and the unchanged merge.
int launch_prefill_attention_padded(const f16* q, const f16* k, const f16* v, f16* out, float* ws, int B, int H, int Hkv, int Tq,
                                    int max_keys, int D, const int64_t* kv_len, int kv_len_bias, const int64_t* kv_start, int splits,
                                    float scaling, const long* st, hipStream_t stream)
{
    PrefillPadArgs a;
    a.kv_start = kv_start;
    auto front = [&] {
        const int rc = check_prefill_common(q, k, v, out, B, H, Hkv, Tq, max_keys, D, st);
        if (rc != EETQ_OK) return rc;
        EETQ_REQUIRE(kv_start, "null kv_start");
        return (int)EETQ_OK;
    };
    return launch_prefill_forms<false, true>(a, front, q, k, v, out, ws, B, H, Hkv, Tq, max_keys, D, kv_len, kv_len_bias, splits, scaling, st,
                                             stream, "prefill_attn_kernel (per-row first key) launch",
                                             "prefill_attn_kernel (per-row first key, split) launch");
}

// launch_prefill_attention_dev with a sliding window (the WIN form above): query t attends the `window` cache rows up to its own.
// Always the device-length kernel (kv_len nullptr: max_keys keys, a fresh prompt), or the split form and the unchanged merge.
int launch_prefill_attention_window(const f16* q, const f16* k, const f16* v, f16* out, float* ws, int B, int H, int Hkv, int Tq,
                                    int max_keys, int D, const int64_t* kv_len, int kv_len_bias, int window, int splits, float scaling,
                                    const long* st, hipStream_t stream)
{
    PrefillWinArgs a;
    a.window = std::min(window, std::max(max_keys, 1));   // (a longer window is the whole prefix; keeps the kernel's 32-bit arithmetic in range)
    auto front = [&] {
        const int rc = check_prefill_common(q, k, v, out, B, H, Hkv, Tq, max_keys, D, st);
        if (rc != EETQ_OK) return rc;
        EETQ_REQUIRE(window >= 1, "the attention window must be at least 1 row");
        return (int)EETQ_OK;
    };
    return launch_prefill_forms<false, false, true>(a, front, q, k, v, out, ws, B, H, Hkv, Tq, max_keys, D, kv_len, kv_len_bias, splits,
                                                    scaling, st, stream, "prefill_attn_kernel (window) launch",
                                                    "prefill_attn_kernel (window, split) launch");
}

// launch_prefill_attention_window over a RING cache of ring_rows rows (the RING form above): logical row r at physical row
// r mod ring_rows; max_keys and kv_len count logical rows.  ring_rows % 64 == 0 and ring_rows >= window + Tq + 62.
int launch_prefill_attention_ring(const f16* q, const f16* k, const f16* v, f16* out, float* ws, int B, int H, int Hkv, int Tq,
                                  int max_keys, int D, const int64_t* kv_len, int kv_len_bias, int window, int ring_rows, int splits,
                                  float scaling, const long* st, hipStream_t stream)
{
    PrefillRingArgs a;
    a.window      = std::min(window, std::max(max_keys, 1));
    a.ring_blocks = ring_rows / kPfBN;
    auto front = [&] {
        EETQ_REQUIRE(ring_rows > 0 && ring_rows % kPfBN == 0, "a ring cache behind the prompt kernel must have a multiple of 64 rows");
        const int rc = check_prefill_common(q, k, v, out, B, H, Hkv, Tq, ring_rows, D, st);
        if (rc != EETQ_OK) return rc;
        EETQ_REQUIRE(window >= 1, "the attention window must be at least 1 row");
        EETQ_REQUIRE(max_keys <= (1 << 30), "max_keys must not exceed 2^30 logical rows");
        EETQ_REQUIRE((long)ring_rows >= (long)window + Tq + 62,
                     "a ring cache behind the prompt kernel must have at least window + query rows + 62 rows (a launch must not read "
                     "key blocks its own rows have replaced)");
        return (int)EETQ_OK;
    };
    return launch_prefill_forms<false, false, true, true>(a, front, q, k, v, out, ws, B, H, Hkv, Tq, max_keys, D, kv_len, kv_len_bias,
                                                          splits, scaling, st, stream, "prefill_attn_kernel (ring) launch",
                                                          "prefill_attn_kernel (ring, split) launch");
}

// launch_prefill_attention_dev over an int8 cache (kv_i8.hpp): st as there with the k / v entries in BYTES, sst {batch, head, row} of
// the scale pairs in fp16 elements.  Always the device-length kernel (kv_len nullptr: max_keys keys), or the split form and the merge.
int launch_prefill_attention_i8kv(const f16* q, const int8_t* k, const int8_t* v, const f16* scales, f16* out, float* ws, int B, int H,
                                  int Hkv, int Tq, int max_keys, int D, const int64_t* kv_len, int kv_len_bias, int splits, float scaling,
                                  const long* st, const long* sst, hipStream_t stream)
{
    EETQ_REQUIRE(q && k && v && scales && out && st && sst, "null pointer");
    PrefillDevArgs8 a;
    a.scales = scales, a.s_sb = sst[0], a.s_sh = sst[1], a.s_ss = sst[2];
    auto front = [&] {
        EETQ_REQUIRE(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && Tq > 0, "invalid attention shape");
        if (!prefill_attention_supports(D)) return fail(EETQ_ERR_UNSUPPORTED, "[eetq_amd] prompt attention supports head_dim 64 and 128");
        for (int i = 0; i < 3; ++i) EETQ_REQUIRE(st[i] % 8 == 0, "q strides must be multiples of 8 elements (16-byte loads)");
        for (int i = 9; i < 12; ++i) EETQ_REQUIRE(st[i] % 4 == 0, "out strides must be multiples of 4 elements");
        EETQ_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)out % 8 == 0, "q must be 16-byte aligned, out 8-byte");
        return check_i8_cache(k, v, scales, max_keys, st + 3, sst);
    };
    return launch_prefill_forms<true, false>(a, front, q, reinterpret_cast<const f16*>(k), reinterpret_cast<const f16*>(v), out, ws, B, H,
                                             Hkv, Tq, max_keys, D, kv_len, kv_len_bias, splits, scaling, st, stream,
                                             "prefill_attn_kernel (int8 rows) launch", "prefill_attn_kernel (int8 rows, split) launch");
}

}  // namespace eetq
