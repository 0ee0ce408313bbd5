// Speculative greedy decoding by n-gram lookup (extension for the HIP-graph decoder, utils/graph_decoder.py):
//   * eetq_spec_ngram_draft_i64: per batch row the longest recent n-gram (n <= max_ngram) that repeats the tail of the row's token
//     history, and the k tokens that followed it -- the draft of one verify pass.  One workgroup per row, ONE pass over the
//     candidate end columns e, reduced on the key (match length, e): the longest match wins, the most recent among equals.
//   * eetq_spec_accept_f16: argmax of the k + 1 verify rows by greedy_handover_kernel's rule (norm_rope.hip), the number of
//     leading draft tokens every batch row confirms, and the hand-over of 1 .. k + 1 tokens: output columns, history columns,
//     next input id, position, column, statistics.  ONE workgroup walks the rows position-major and stops at the first
//     position a row rejects: the entry has no workspace argument to carry argmaxes between workgroups, a rejected draft costs
//     what greedy_handover costs, and the counters are read before anyone advances them, as there.
// Plain C++: vector stores only, no atomics, deterministic.  Both launches are capturable: nothing is allocated or read on the host.
#include "common.hpp"

namespace eetq {

namespace {

typedef unsigned long long u64;

constexpr int kThreads  = 1024;
constexpr int kWaves    = kThreads / 64;
constexpr int kMaxNgram = 8;
constexpr int kMaxDraft = 15;

// monotone 16-bit key of an fp16 value, every NaN above +inf, -0 and +0 share one (greedy_handover_kernel's key_of)
__device__ __forceinline__ u32 key16(f16 v)
{
    const unsigned short u = __builtin_bit_cast(unsigned short, v);
    return ((u & 0x7FFF) > 0x7C00) ? 0xFFFFu : ((u & 0x7FFF) == 0) ? 0x8000u : (u & 0x8000) ? (u32)(unsigned short)~u : (u32)(u | 0x8000);
}

// the workgroup's maximum of `v`; `slot`: kWaves words of LDS.  Every thread returns it.
__device__ __forceinline__ u64 block_max(u64 v, u64* slot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 o = __shfl_xor(v, m, 64);
        v           = o > v ? o : v;
    }
    __syncthreads();  // slot may still be read by the previous reduction
    if (lane == 0) slot[wave] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v = slot[w] > v ? slot[w] : v;
    return v;
}

// torch.argmax's answer for one row: the first index of the maximum, a NaN counts as the maximum.  16-byte loads wherever the
// address allows, whatever the row's alignment (an odd vocab puts every second row on a 2-byte boundary).
__device__ int argmax_row(const f16* __restrict__ row, int vocab, u64* slot)
{
    const int tid  = threadIdx.x;
    u64       best = 0;
    auto      take = [&](f16 v, int i) {
        const u64 k = ((u64)key16(v) << 32) | (u32)(0xFFFFFFFFu - (u32)i);
        best        = k > best ? k : best;
    };
    int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1);
    head     = head < vocab ? head : vocab;
    if (tid < head) take(row[tid], tid);
    const int nvec = (vocab - head) >> 3;
    for (int i = tid; i < nvec; i += kThreads) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(row + head + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) take(v[j], head + i * 8 + j);
    }
    const int tb = head + nvec * 8;
    if (tid < vocab - tb) take(row[tb + tid], tb + tid);
    best          = block_max(best, slot);
    const u32 tok = 0xFFFFFFFFu - (u32)(best & 0xFFFFFFFFu);
    return tok < (u32)vocab ? (int)tok : 0;
}

__global__ __launch_bounds__(kThreads) void ngram_draft_kernel(const int64_t* __restrict__ hist, long hist_stride, int cols,
                                                               const int64_t* __restrict__ position, int max_ngram, int k,
                                                               int64_t* __restrict__ draft, long draft_stride)
{
    __shared__ u64 slot[kWaves];
    const int      tid = threadIdx.x;
    const int64_t* row = hist + (long)blockIdx.x * hist_stride;
    const int64_t  p   = *position;
    const int      L   = p + 1 < 1 ? 1 : p + 1 > (int64_t)cols ? cols : (int)(p + 1);   // tokens of the row; the last is pending
    const int      nmax = max_ngram < L - 1 ? max_ngram : L - 1;
    int64_t        tail[kMaxNgram];   // tail[j] = row[L - 1 - j]
#pragma unroll
    for (int j = 0; j < kMaxNgram; ++j) tail[j] = j < nmax ? row[L - 1 - j] : 0;
    // key = match length << 32 | e for a candidate with at least one matching token, 0 otherwise
    u64 best = 0;
    for (int e = tid; e <= L - 2; e += kThreads) {
        const int lim = nmax < e + 1 ? nmax : e + 1;   // the n-gram may not start before column 0
        int       m   = 0;
#pragma unroll
        for (int j = 0; j < kMaxNgram; ++j) {
            if (j >= lim || row[e - j] != tail[j]) break;
            m = j + 1;
        }
        const u64 key = m ? ((u64)m << 32) | (u32)e : 0ull;
        best          = key > best ? key : best;
    }
    best = block_max(best, slot);
    if (tid < k) {
        int64_t tok;
        if (best == 0) {
            tok = row[L - 1];
        } else {
            // ext = row[0 .. L - 1] followed by the draft itself: draft[i] = ext[e + 1 + i] repeats row[e + 1 .. L - 1]
            const int e = (int)(u32)best, period = L - 1 - e;
            tok         = row[e + 1 + tid % period];
        }
        draft[(long)blockIdx.x * draft_stride + tid] = tok;
    }
}

__global__ __launch_bounds__(kThreads) void spec_accept_kernel(const f16* __restrict__ logits, long stride_b, long stride_t, int vocab,
                                                               int batch, int k, const int64_t* __restrict__ draft, long draft_stride,
                                                               int64_t* __restrict__ out_buf, long out_stride, int out_cols,
                                                               int64_t* __restrict__ s_idx, int64_t* __restrict__ s_pos,
                                                               const int64_t* __restrict__ s_limit, int64_t* __restrict__ s_tok,
                                                               long tok_stride, int64_t* __restrict__ hist, long hist_stride,
                                                               int hist_cols, int64_t* __restrict__ stats)
{
    __shared__ u64 slot[kWaves];
    __shared__ int rejected;
    const int      tid = threadIdx.x;
    const int64_t  col = *s_idx, pos = *s_pos, room = *s_limit - col;
    // adv = clamp(min(n + 1, room), 0, k + 1): positions at or beyond `want` can never be handed over and are not read
    const int want = room < 0 ? 0 : room > (int64_t)(k + 1) ? k + 1 : (int)room;
    int       adv  = 0;
    if (tid == 0) rejected = 0;
    __syncthreads();
    // Position t is reached only when every row confirmed draft[0 .. t - 1], so t <= n: its token is handed over whatever its own
    // verdict.  The next input id is the token of the last position reached (each position overwrites the one before).
    for (int t = 0; t < want; ++t) {
        for (int b = 0; b < batch; ++b) {
            const int tok = argmax_row(logits + b * stride_b + t * stride_t, vocab, slot);
            if (tid == 0) {
                const int64_t oc = col + t, hc = pos + 1 + t;
                if (oc >= 0 && oc < out_cols) out_buf[b * out_stride + oc] = tok;
                if (hc >= 0 && hc < hist_cols) hist[b * hist_stride + hc] = tok;
                s_tok[b * tok_stride] = tok;
                if (t < k && draft[b * draft_stride + t] != (int64_t)tok) rejected = 1;
            }
        }
        adv = t + 1;
        __syncthreads();
        if (rejected) break;   // one row's rejection ends the step for all of them: they share one cache counter
    }
    if (tid == 0) {
        *s_pos   = pos + adv;
        *s_idx   = col + adv;
        stats[0] = stats[0] + 1;
        stats[1] = stats[1] + adv;
    }
}

}  // namespace

int launch_spec_ngram_draft(const int64_t* hist, long hist_stride, int cols, int batch, const int64_t* position, int max_ngram, int k,
                            int64_t* draft, long draft_stride, hipStream_t stream)
{
    EETQ_REQUIRE(hist, "spec_ngram_draft: hist is null");
    EETQ_REQUIRE(position, "spec_ngram_draft: position is null");
    EETQ_REQUIRE(draft, "spec_ngram_draft: draft is null");
    EETQ_REQUIRE(max_ngram >= 1 && max_ngram <= kMaxNgram, "spec_ngram_draft: max_ngram must lie in 1 .. 8");
    EETQ_REQUIRE(k >= 1 && k <= kMaxDraft, "spec_ngram_draft: k must lie in 1 .. 15");
    EETQ_REQUIRE(batch > 0, "spec_ngram_draft: batch must be positive");
    EETQ_REQUIRE(cols > 0, "spec_ngram_draft: cols must be positive");
    EETQ_REQUIRE(hist_stride >= cols, "spec_ngram_draft: the history's row stride must be at least cols");
    EETQ_REQUIRE(draft_stride >= k, "spec_ngram_draft: the draft's row stride must be at least k");
    EETQ_REQUIRE((uintptr_t)hist % 8 == 0 && (uintptr_t)position % 8 == 0 && (uintptr_t)draft % 8 == 0,
                 "spec_ngram_draft: int64 pointers must be 8-byte aligned");
    ngram_draft_kernel<<<batch, kThreads, 0, stream>>>(hist, hist_stride, cols, position, max_ngram, k, draft, draft_stride);
    return check_hip(hipGetLastError(), "ngram_draft_kernel launch");
}

int launch_spec_accept(const f16* logits, long stride_b, long stride_t, int vocab, int batch, int k, const int64_t* draft,
                       long draft_stride, int64_t* out_buf, long out_stride, int out_cols, int64_t* s_idx, int64_t* s_pos,
                       const int64_t* s_limit, int64_t* s_tok, long tok_stride, int64_t* hist, long hist_stride, int hist_cols,
                       int64_t* stats, hipStream_t stream)
{
    EETQ_REQUIRE(logits, "spec_accept: logits is null");
    EETQ_REQUIRE(draft, "spec_accept: draft is null");
    EETQ_REQUIRE(out_buf, "spec_accept: out_tokens is null");
    EETQ_REQUIRE(s_idx, "spec_accept: column is null");
    EETQ_REQUIRE(s_pos, "spec_accept: position is null");
    EETQ_REQUIRE(s_limit, "spec_accept: limit is null");
    EETQ_REQUIRE(s_tok, "spec_accept: next_token is null");
    EETQ_REQUIRE(hist, "spec_accept: hist is null");
    EETQ_REQUIRE(stats, "spec_accept: stats is null");
    EETQ_REQUIRE(k >= 1 && k <= kMaxDraft, "spec_accept: k must lie in 1 .. 15");
    EETQ_REQUIRE(vocab > 0, "spec_accept: vocab must be positive");
    EETQ_REQUIRE(batch > 0, "spec_accept: batch must be positive");
    EETQ_REQUIRE(stride_t >= vocab, "spec_accept: the logits' position stride must be at least vocab");
    EETQ_REQUIRE(stride_b >= vocab, "spec_accept: the logits' batch stride must be at least vocab");
    EETQ_REQUIRE(draft_stride >= k, "spec_accept: the draft's row stride must be at least k");
    EETQ_REQUIRE(out_cols > 0 && out_stride >= out_cols, "spec_accept: out_stride must be at least out_cols, out_cols positive");
    EETQ_REQUIRE(hist_cols > 0 && hist_stride >= hist_cols, "spec_accept: the history's row stride must be at least cols, cols positive");
    EETQ_REQUIRE(tok_stride >= 1, "spec_accept: next_token's row stride must be at least 1");
    EETQ_REQUIRE((uintptr_t)draft % 8 == 0 && (uintptr_t)out_buf % 8 == 0 && (uintptr_t)s_idx % 8 == 0 && (uintptr_t)s_pos % 8 == 0 &&
                     (uintptr_t)s_limit % 8 == 0 && (uintptr_t)s_tok % 8 == 0 && (uintptr_t)hist % 8 == 0 && (uintptr_t)stats % 8 == 0,
                 "spec_accept: int64 pointers must be 8-byte aligned");
    EETQ_REQUIRE((uintptr_t)logits % 2 == 0, "spec_accept: logits must be 2-byte aligned");
    spec_accept_kernel<<<1, kThreads, 0, stream>>>(logits, stride_b, stride_t, vocab, batch, k, draft, draft_stride, out_buf, out_stride,
                                                   out_cols, s_idx, s_pos, s_limit, s_tok, tok_stride, hist, hist_stride, hist_cols, stats);
    return check_hip(hipGetLastError(), "spec_accept_kernel launch");
}

}  // namespace eetq

extern "C" {

int eetq_spec_ngram_draft_i64(const int64_t* hist, long hist_stride, int cols, int batch, const int64_t* position, int max_ngram, int k,
                              int64_t* draft, long draft_stride, void* stream)
{
    return eetq::launch_spec_ngram_draft(hist, hist_stride, cols, batch, position, max_ngram, k, draft, draft_stride,
                                         static_cast<hipStream_t>(stream));
}

int eetq_spec_accept_f16(const void* logits, long stride_b, long stride_t, int vocab, int batch, int k, const int64_t* draft,
                         long draft_stride, int64_t* out_tokens, long out_stride, int out_cols, int64_t* column, int64_t* position,
                         const int64_t* limit, int64_t* next_token, long next_stride, int64_t* hist, long hist_stride, int hist_cols,
                         int64_t* stats, void* stream)
{
    return eetq::launch_spec_accept(static_cast<const eetq::f16*>(logits), stride_b, stride_t, vocab, batch, k, draft, draft_stride,
                                    out_tokens, out_stride, out_cols, column, position, limit, next_token, next_stride, hist,
                                    hist_stride, hist_cols, stats, static_cast<hipStream_t>(stream));
}

}  // extern "C"
