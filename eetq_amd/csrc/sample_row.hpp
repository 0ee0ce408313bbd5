// The token of ONE row of fp16 logits by one workgroup of 1024 threads: temperature, top-k, top-p and the draw
// (sample_row), the argmax (greedy_row), the row visitor, the scans, Philox and the 32-byte parameter block.  Device code shared by
// sample.hip (one row per batch row, eetq_sample_handover_f16) and spec_sample.hip (one row per (batch row, verify position),
// eetq_spec_sample_accept_f16); everything has internal linkage.  No sort: fp16 logits have at most 65 536 distinct values, so
// everything is a threshold search over VALUE CLASSES:
//   * the 16-bit monotone key of a logit (greedy_handover_kernel's key_of; a NaN takes the key of -inf) splits into a coarse
//     bin (key >> 6, 1024 of them) and 64 fine classes;
//   * the weight of a class is count * q(key), q = floor(exp((value - max) / temperature) * 2^40) -- an INTEGER, so every
//     cumulative sum is exact whatever the order of the LDS atomics that build it, the same in every pass, and a bin's mass is
//     exactly the sum of its classes' (error against real arithmetic: the fp32 exp's, ~2^-18 relative);
//   * pass A: coarse counts + the row's maximum; pass B: coarse masses + the fine counts of the bin that holds the k-th value;
//     pass C: fine counts of the bin the p-cut falls in; pass D: fine counts, per wave segment of the row, of the bin the draw
//     falls in.  The j-th member (by index) of the drawn class is then found from the segment counts and two short scans.
#pragma once
#include "common.hpp"

namespace eetq {

namespace {

typedef unsigned long long u64;
typedef unsigned __int128  u128;

constexpr int kThreads = 1024;
constexpr int kWaves   = kThreads / 64;
constexpr u32 kKeyNegInf = 0x03FFu, kKeyPosInf = 0xFC00u;
constexpr int kTicketShift = 40;   // bits 40.. of *position count the finished rows during a launch: -2^39 <= *position < 2^39

struct SampleParams {  // the 32-byte device block of eetq_sample_handover_f16
    float temperature, top_p;
    int   top_k, eos_token, pad_token, reserved;
    u64   seed;
};
static_assert(sizeof(SampleParams) == 32, "parameter block layout");

// monotone 16-bit key of an fp16 value (-0 and +0 share one); every NaN becomes `nan_key`
__device__ __forceinline__ u32 key16(f16 v, u32 nan_key)
{
    const unsigned short u = __builtin_bit_cast(unsigned short, v);
    return ((u & 0x7FFF) > 0x7C00) ? nan_key : ((u & 0x7FFF) == 0) ? 0x8000u : (u & 0x8000) ? (u32)(unsigned short)~u : (u32)(u | 0x8000);
}

__device__ __forceinline__ float value_of_key(u32 key)
{
    const unsigned short u = key >= 0x8000u ? (unsigned short)(key & 0x7FFF) : (unsigned short)~key;
    return (float)__builtin_bit_cast(f16, u);
}

// fixed-point weight of a class: floor(exp((v - vmax) / T) * one), one = 2^40 (2^32 for a row of more than 2^23 entries, so
// that the sum of a row's weights stays below 2^63); `one` for the maximum itself, 0 for -inf and below e^-30
__device__ __forceinline__ float weight_one(int vocab) { return vocab <= (1 << 23) ? 0x1p40f : 0x1p32f; }
__device__ __forceinline__ u64 weight_of_key(u32 key, float vmax, float temperature, float one)
{
    const float x = (value_of_key(key) - vmax) / temperature;
    return (x > -30.f) ? (u64)(expf(fminf(x, 0.f)) * one) : 0ull;
}

// elements [begin, end) of a row by `n` threads (this one is `t`): 16-byte loads wherever the address allows, whatever the
// row's alignment; f(value, index).  At most 7 scalar elements on either side.
template <typename F>
__device__ __forceinline__ void visit(const f16* __restrict__ row, int begin, int end, int t, int n, F f)
{
    int head = (int)(((16 - ((uintptr_t)(row + begin) & 15)) & 15) >> 1);
    head     = head < end - begin ? head : end - begin;
    if (t < head) f(row[begin + t], begin + t);
    const int vb = begin + head, nvec = (end - vb) >> 3;
    for (int i = t; i < nvec; i += n) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(row + vb + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) f(v[j], vb + i * 8 + j);
    }
    const int tb = vb + nvec * 8;
    if (t < end - tb) f(row[tb + t], tb + t);
}

__device__ __forceinline__ u64 wave_incl_scan(u64 v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive prefix of v in thread order over the workgroup; *total = the sum.  `red`: kWaves words of LDS.
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64* red, u64* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 inc  = wave_incl_scan(v, lane);
    __syncthreads();  // red may still be read by the previous scan
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    // the 16 wave totals, scanned in every wave by its own lanes (lane l holds wave l & 15's)
    const u64 r   = red[lane & (kWaves - 1)];
    u64       acc = r;
#pragma unroll
    for (int d = 1; d < kWaves; d <<= 1) {
        const u64 o = __shfl_up(acc, d, 64);
        if ((lane & (kWaves - 1)) >= d) acc += o;
    }
    *total           = __shfl(acc, kWaves - 1, 64);
    const u64 before = __shfl(acc - r, wave, 64);
    return before + inc - v;
}

struct Philox {
    u32 x[4];
};
__device__ __forceinline__ Philox philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
        c1 = (u32)p1;
        c3 = (u32)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox{{c0, c1, c2, c3}};
}

struct Lds {
    u64 mass[1024];          // per coarse bin; thread t owns bin 1023 - t (descending value order = thread order)
    u32 cnt[1024];
    u32 fine[kWaves][64];    // fine counts of ONE coarse bin, per wave (pass D: per wave segment of the row)
    u64 red[kWaves];
    u64 best[kWaves];
    u64 w64[4];              // broadcast slots
    int w32[8];
};

// fine counts of coarse bin `bin`: wave w counts its segment [w * seg, (w + 1) * seg) of the row into fine[w]
__device__ __forceinline__ void fine_pass(const f16* __restrict__ row, int vocab, int seg, u32 bin, Lds& s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s.fine[wave][lane] = 0;  // (own wave's row: the wave's LDS operations are in order)
    __syncthreads();
    const int b0 = wave * seg < vocab ? wave * seg : vocab, b1 = b0 + seg < vocab ? b0 + seg : vocab;
    visit(row, b0, b1, lane, 64, [&](f16 v, int) {
        const u32 k = key16(v, kKeyNegInf);
        if ((k >> 6) == bin) atomicAdd(&s.fine[wave][k & 63], 1u);
    });
    __syncthreads();
}

// The token of one row for temperature > 0 (DESIGN.md 4.15 has the contract); every thread returns it.
__device__ int sample_row(const f16* __restrict__ row, int vocab, float temperature, float top_p, int top_k, u32 m_u, Lds& s)
{
    const int  tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool use_k = top_k > 0 && top_k < vocab;
    const bool use_p = top_p > 0.f && top_p < 1.f;
    const int  seg   = (vocab + kWaves - 1) / kWaves;
    const u32  mybin = 1023u - (u32)tid;

    // ---- pass A: the maximum (NaN = -inf) and, for top-k, the coarse counts
    s.cnt[tid]  = 0;
    s.mass[tid] = 0;
    __syncthreads();
    u32 kmax = 0;
    visit(row, 0, vocab, tid, kThreads, [&](f16 v, int) {
        const u32 k = key16(v, kKeyNegInf);
        kmax        = k > kmax ? k : kmax;
        if (use_k) atomicAdd(&s.cnt[k >> 6], 1u);
    });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u32 o = __shfl_xor(kmax, m, 64);
        kmax        = o > kmax ? o : kmax;
    }
    if (lane == 0) s.red[wave] = kmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) kmax = (u32)s.red[w] > kmax ? (u32)s.red[w] : kmax;
    if (kmax <= kKeyNegInf) return 0;  // nothing above -inf
    u64 total;
    if (kmax == kKeyPosInf) {          // the first index holding +inf
        u32 first = 0xFFFFFFFFu;
        visit(row, 0, vocab, tid, kThreads, [&](f16 v, int i) {
            if (key16(v, kKeyNegInf) == kKeyPosInf) first = (u32)i < first ? (u32)i : first;
        });
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const u32 o = __shfl_xor(first, m, 64);
            first       = o < first ? o : first;
        }
        __syncthreads();
        if (lane == 0) s.red[wave] = first;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) first = (u32)s.red[w] < first ? (u32)s.red[w] : first;
        return (int)first;
    }
    const float vmax = value_of_key(kmax), one = weight_one(vocab);

    // ---- top-k, coarse: the bin that holds the k-th largest value
    u32 kbin = 0, kbefore = 0;  // entries in the bins above kbin
    if (use_k) {
        const u32 c      = s.cnt[mybin];
        const u32 before = (u32)block_excl_scan(c, s.red, &total);
        if (before < (u32)top_k && (u32)top_k <= before + c) {
            s.w32[0] = (int)mybin;
            s.w32[1] = (int)before;
        }
        __syncthreads();
        kbin    = (u32)s.w32[0];
        kbefore = (u32)s.w32[1];
    }

    // ---- pass B: coarse masses (integers: exact in any order) + the fine counts of kbin
    s.fine[wave][lane] = 0;
    __syncthreads();
    visit(row, 0, vocab, tid, kThreads, [&](f16 v, int) {
        const u32 k = key16(v, kKeyNegInf);
        const u64 q = weight_of_key(k, vmax, temperature, one);
        if (q) atomicAdd(&s.mass[k >> 6], q);
        if (use_k && (k >> 6) == kbin) atomicAdd(&s.fine[0][k & 63], 1u);
    });
    __syncthreads();

    // ---- top-k, fine: the threshold key tk (ties at the threshold all stay) and what survives of kbin's mass
    u32 tk = 0;
    if (use_k) {
        if (wave == 0) {
            const u32 f   = 63u - (u32)lane;  // descending
            const u32 c   = s.fine[0][f];
            const u64 inc = wave_incl_scan(c, lane);
            const bool kept = kbefore + (inc - c) < (u64)top_k;   // fewer than k entries are strictly larger
            const u64  m    = kept ? (u64)c * weight_of_key(kbin * 64 + f, vmax, temperature, one) : 0ull;
            const u64  minc = wave_incl_scan(m, lane);
            const u64  ball = __ballot(kept && c > 0);
            if (lane == 63) s.w64[0] = minc;
            if (lane == 0) s.w32[0] = (int)(kbin * 64 + (63u - (u32)(63 - __builtin_clzll(ball | 1ull))));
        }
        __syncthreads();
        tk = (u32)s.w32[0];
        if (mybin == kbin) s.mass[mybin] = s.w64[0];
        if (mybin < kbin) s.mass[mybin] = 0;
        __syncthreads();
    }
    u64 sum_k;
    u64 before = block_excl_scan(s.mass[mybin], s.red, &sum_k);

    // ---- top-p: a class stays iff the mass of the strictly larger classes is < p * sum_k
    u32 tp = tk;
    u64 sum_p = sum_k;
    if (use_p) {
        u64 m_p = (u64)((double)top_p * 4294967296.0);   // p in 2^-32 steps, never 0: the top class always stays
        m_p     = m_p ? m_p : 1;
        const u128 cut  = (u128)sum_k * m_p;
        const bool here = ((u128)before << 32) < cut;
        const u64  mine = s.mass[mybin];
        // the lowest bin whose first class may still stay (a prefix in descending order)
        if (here && (tid == kThreads - 1 || !(((u128)(before + mine) << 32) < cut))) {
            s.w32[0] = (int)mybin;
            s.w64[0] = before;
        }
        __syncthreads();
        const u32 pbin    = (u32)s.w32[0];
        const u64 pbefore = s.w64[0];
        __syncthreads();
        fine_pass(row, vocab, seg, pbin, s);   // ---- pass C
        if (wave == 0) {
            const u32 f = 63u - (u32)lane;
            u32       c = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) c += s.fine[w][f];
            const u32  key  = pbin * 64 + f;
            const u64  m    = key >= tk ? (u64)c * weight_of_key(key, vmax, temperature, one) : 0ull;
            const u64  inc  = wave_incl_scan(m, lane);
            const bool kept = key >= tk && (((u128)(pbefore + inc - m) << 32) < cut);
            const u64  kinc = wave_incl_scan(kept ? m : 0ull, lane);
            const u64  ball = __ballot(kept && c > 0);
            if (lane == 63) s.w64[1] = kinc;
            // lowest kept class that has members; none (an empty stretch): keep the bins above only
            if (lane == 0) s.w32[1] = ball ? (int)(pbin * 64 + (63u - (u32)(63 - __builtin_clzll(ball)))) : (int)(pbin * 64 + 64);
        }
        __syncthreads();
        tp = (u32)s.w32[1] > tk ? (u32)s.w32[1] : tk;
        if (mybin == pbin) s.mass[mybin] = s.w64[1];
        if (mybin < pbin) s.mass[mybin] = 0;
        __syncthreads();
        before = block_excl_scan(s.mass[mybin], s.red, &sum_p);
    }

    // ---- the draw: the first class (value descending) whose cumulative mass exceeds u * sum_p, u = m_u / 2^24
    const u128 x = (u128)sum_p * m_u;
    {
        const u64 mine = s.mass[mybin];
        if (!(((u128)before << 24) > x) && (((u128)(before + mine) << 24) > x)) {
            s.w32[2] = (int)mybin;
            s.w64[2] = before;
        }
    }
    __syncthreads();
    const u32 dbin    = (u32)s.w32[2];
    const u64 dbefore = s.w64[2];
    __syncthreads();
    fine_pass(row, vocab, seg, dbin, s);   // ---- pass D
    if (wave == 0) {
        const u32 f = 63u - (u32)lane;
        u32       c = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) c += s.fine[w][f];
        const u32  key = dbin * 64 + f;
        const u64  q   = key >= tp ? weight_of_key(key, vmax, temperature, one) : 0ull;
        const u64  m   = (u64)c * q;
        const u64  inc = wave_incl_scan(m, lane);
        const bool hit = !(((u128)(dbefore + inc - m) << 24) > x) && (((u128)(dbefore + inc) << 24) > x);
        if (hit) {  // exactly one lane: the sums are exact
            const u64 r = (u64)((x - ((u128)(dbefore + inc - m) << 24)) >> 24);
            u64       j = r / q;   // the first j with (j + 1) q 2^24 > x - before 2^24
            j           = j < c ? j : c - 1;
            s.w32[3]    = (int)key;
            s.w32[4]    = (int)j;
        }
    }
    __syncthreads();
    const u32 dkey = (u32)s.w32[3];
    u32       j    = (u32)s.w32[4];

    // ---- the j-th member of the class by index: wave segment from pass D's counts, 1/16 of it, then a ballot scan
    int lo = 0, hi = 0;
    {
        u32 acc = 0;
        int w   = 0;
        for (; w < kWaves - 1; ++w) {
            const u32 c = s.fine[w][dkey & 63];
            if (j < acc + c) break;
            acc += c;
        }
        j -= acc;
        lo = w * seg < vocab ? w * seg : vocab;
        hi = lo + seg < vocab ? lo + seg : vocab;
    }
    __syncthreads();
    {
        const int sub = (hi - lo + kWaves - 1) / kWaves;
        const int b0 = lo + wave * sub < hi ? lo + wave * sub : hi, b1 = b0 + sub < hi ? b0 + sub : hi;
        u32       c  = 0;
        for (int i = b0 + lane; i < b1; i += 64) c += key16(row[i], kKeyNegInf) == dkey;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
        if (lane == 0) s.red[wave] = c;
        __syncthreads();
        u32 acc = 0;
        int w   = 0;
        for (; w < kWaves - 1; ++w) {
            const u32 cw = (u32)s.red[w];
            if (j < acc + cw) break;
            acc += cw;
        }
        j -= acc;
        lo = lo + w * sub < hi ? lo + w * sub : hi;
        hi = lo + sub < hi ? lo + sub : hi;
    }
    __syncthreads();
    if (wave == 0) {
        int tok = hi > lo ? hi - 1 : (vocab - 1);
        for (int i0 = lo; i0 < hi; i0 += 64) {
            const int  i     = i0 + lane;
            const bool match = i < hi && key16(row[i], kKeyNegInf) == dkey;
            const u64  ball  = __ballot(match);
            const u32  c     = (u32)__builtin_popcountll(ball);
            if (j < c) {
                u64 b = ball;
                for (u32 n = 0; n < j; ++n) b &= b - 1;   // drop the j lowest matches
                tok = i0 + __builtin_ctzll(b);
                break;
            }
            j -= c;
        }
        if (lane == 0) s.w32[5] = tok;
    }
    __syncthreads();
    const int tok = s.w32[5];
    return tok < 0 ? 0 : tok < vocab ? tok : vocab - 1;
}

// torch.argmax's answer: the first index of the maximum, a NaN counts as the maximum (greedy_handover_kernel's rule)
__device__ int greedy_row(const f16* __restrict__ row, int vocab, Lds& s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64       best = 0;
    visit(row, 0, vocab, tid, kThreads, [&](f16 v, int i) {
        const u64 k = ((u64)key16(v, 0xFFFFu) << 32) | (u32)(0xFFFFFFFFu - (u32)i);
        best        = k > best ? k : best;
    });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 o = __shfl_xor(best, m, 64);
        best        = o > best ? o : best;
    }
    if (lane == 0) s.best[wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) best = s.best[w] > best ? s.best[w] : best;
    const u32 tok = 0xFFFFFFFFu - (u32)(best & 0xFFFFFFFFu);
    return tok < (u32)vocab ? (int)tok : 0;
}

}  // namespace

}  // namespace eetq
