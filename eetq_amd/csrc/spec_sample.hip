// Speculative decoding for sampled generation (extension for the HIP-graph decoder, utils/graph_decoder.py):
// eetq_spec_sample_accept_f16 = the verify / accept / hand-over of eetq_spec_accept_f16 (spec.hip) with every row's token drawn as
// eetq_sample_handover_f16 (sample.hip) draws it -- temperature / top-k / top-p, Philox per (column, row), EOS flags.  A draft
// token is a point mass, so "draw x from the target distribution, accept iff x == draft, hand x over either way" IS exact
// speculative sampling, and the token at an output column is the same function of (logits, seed, column, row) as without a draft.
//   * ONE workgroup per (batch row, verify position): the k + 1 rows of a batch row are independent until the accept, so they run
//     on batch * (k + 1) CUs at once (sample_row.hpp's device code, unchanged) instead of in series;
//   * lane 0 publishes the token to workspace[b * (k + 1) + t] (agent-scope atomic store), then takes a ticket (agent-scope
//     acq_rel fetch_add).  The ticket lives where sample_handover_kernel keeps it: bits 40.. of *position, biased by 2^39, for the
//     length of the launch -- no state between launches, no memset node, no poisoned first launch;
//   * the workgroup that finds batch * (k + 1) - 1 tickets is the last one: it reads the tokens (agent-scope atomic loads behind
//     its lane 0's acquire and a barrier), walks them, hands over, advances the counters and takes the tickets out again.
// Nobody waits for anybody: a grid larger than the chip cannot deadlock.  *column, *limit and done[b] are read by ONE lane per
// workgroup, before its ticket, and written by the last arriver only -- behind every ticket.
#include "sample_row.hpp"

namespace eetq {

namespace {

constexpr int kMaxDraft = 15;

__global__ __launch_bounds__(kThreads) void spec_sample_accept_kernel(
    const f16* __restrict__ logits, long stride_b, long stride_t, int vocab, int batch, int k, const int64_t* __restrict__ draft,
    long draft_stride, int64_t* out_buf, long out_stride, int out_cols, int64_t* s_idx, int64_t* s_pos, const int64_t* s_limit,
    int64_t* s_tok, long tok_stride, int64_t* hist, long hist_stride, int hist_cols, int64_t* stats,
    const SampleParams* __restrict__ params, int* done, const float* __restrict__ uniforms, long uniforms_stride, int64_t* workspace)
{
    __shared__ Lds     s;
    const int          tid = threadIdx.x, T = k + 1, total = batch * T;
    const int          b = (int)blockIdx.x / T, t = (int)blockIdx.x - b * T;   // one workgroup per (row, position)
    const SampleParams p = *params;
    // One lane reads the counters and the row's flag and hands them to the workgroup: the lane that reads is the lane that takes
    // the ticket, so the reads are over (their values went through LDS) before the last arriver may overwrite what they read,
    // and every wave takes the same branches below whatever happens to the counters meanwhile.
    if (tid == 0) {
        const int64_t c = __hip_atomic_load(s_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int64_t room = __hip_atomic_load(s_limit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - c;
        s.w64[3] = (u64)c;
        s.w32[6] = room < 0 ? 0 : room > (int64_t)T ? T : (int)room;   // want: positions at or beyond it are not read
        s.w32[7] = done ? (__hip_atomic_load(done + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) : 0;
    }
    __syncthreads();
    const int64_t col  = (int64_t)s.w64[3];
    const int     want = s.w32[6];
    int64_t       tok  = 0;
    if (t < want && !s.w32[7]) {   // (a row finished at entry hands on pads: its logits are not looked at)
        const f16* row = logits + (long)b * stride_b + (long)t * stride_t;
        if (p.temperature > 0.f) {   // 0, negative and NaN select greedy
            const u64 c = (u64)(col + t);
            u32       m_u;
            if (uniforms) {
                const float u = uniforms[(long)b * uniforms_stride + t];
                m_u           = !(u > 0.f) ? 0u : u >= 1.f ? 0xFFFFFFu : (u32)(u * 16777216.f);
            } else {
                m_u = philox4x32_10((u32)c, (u32)(c >> 32), (u32)b, 0u, (u32)p.seed, (u32)(p.seed >> 32)).x[0] >> 8;
            }
            tok = sample_row(row, vocab, p.temperature, p.top_p, p.top_k, m_u, s);
        } else {
            tok = greedy_row(row, vocab, s);
        }
    }
    __syncthreads();   // the slots written next may still be read (want, and the tails of sample_row / greedy_row)
    if (tid == 0) {
        if (t < want) __hip_atomic_store(workspace + blockIdx.x, tok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u64 old    = __hip_atomic_fetch_add(reinterpret_cast<u64*>(s_pos), 1ull << kTicketShift, __ATOMIC_ACQ_REL,
                                                  __HIP_MEMORY_SCOPE_AGENT);
        const u64 biased = old + (1ull << (kTicketShift - 1));   // tickets count from 0 for a negative position as well
        s.w32[6] = ((biased >> kTicketShift) & 0xFFFFFFull) == (u64)(total - 1);
        s.w64[3] = (biased & ((1ull << kTicketShift) - 1)) - (1ull << (kTicketShift - 1));   // *position itself
    }
    __syncthreads();
    if (!s.w32[6]) return;

    // ---- the last arriver: every token is published (each ticket released its store, lane 0 acquired them all, the barrier
    // above hands that on to the other waves; the loads are agent-scope atomics, which no CU-local cache serves)
    const int64_t pos = (int64_t)s.w64[3], pad = (int64_t)p.pad_token, eos = (int64_t)p.eos_token;
    // the walk, one thread per batch row: the first position at which the row objects
    int adv = want;
    for (int r = tid; r < batch; r += kThreads) {
        bool fin = done && done[r] != 0;
        for (int j = 0; j < want && j < k; ++j) {
            const int64_t x = __hip_atomic_load(workspace + r * T + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t y = fin ? pad : x;
            if (eos >= 0 && y == eos) fin = true;
            if (!fin && draft[r * draft_stride + j] != y) {   // a finished row never objects
                adv = j + 1 < adv ? j + 1 : adv;
                break;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = __shfl_xor(adv, m, 64);
        adv         = o < adv ? o : adv;
    }
    if ((tid & 63) == 0) s.red[tid >> 6] = (u64)adv;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) adv = (int)s.red[w] < adv ? (int)s.red[w] : adv;
    // the hand-over of positions 0 .. adv - 1
    for (int r = tid; r < batch && adv > 0; r += kThreads) {
        bool    fin = done && done[r] != 0;
        int64_t y   = 0;
        for (int j = 0; j < adv; ++j) {
            const int64_t x = __hip_atomic_load(workspace + r * T + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            y               = fin ? pad : x;
            if (eos >= 0 && y == eos) fin = true;
            const int64_t oc = col + j, hc = pos + 1 + j;
            if (oc >= 0 && oc < out_cols) out_buf[r * out_stride + oc] = y;
            if (hc >= 0 && hc < hist_cols) hist[r * hist_stride + hc] = y;
        }
        s_tok[r * tok_stride] = y;
        if (done) done[r] = fin ? 1 : 0;   // as of position adv - 1: an EOS drawn beyond it finishes nothing
    }
    if (tid == 0) {
        __hip_atomic_fetch_add(reinterpret_cast<u64*>(s_pos), (u64)adv - ((u64)total << kTicketShift), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        if (adv > 0) __hip_atomic_store(s_idx, col + adv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stats[0] = stats[0] + 1;
        stats[1] = stats[1] + adv;
    }
}

}  // namespace

int launch_spec_sample_accept(const f16* logits, long stride_b, long stride_t, int vocab, int batch, int k, const int64_t* draft,
                              long draft_stride, int64_t* out_buf, long out_stride, int out_cols, int64_t* s_idx, int64_t* s_pos,
                              const int64_t* s_limit, int64_t* s_tok, long tok_stride, int64_t* hist, long hist_stride, int hist_cols,
                              int64_t* stats, const void* params, int* done, const float* uniforms, long uniforms_stride,
                              int64_t* workspace, hipStream_t stream)
{
    EETQ_REQUIRE(logits, "spec_sample_accept: logits is null");
    EETQ_REQUIRE(draft, "spec_sample_accept: draft is null");
    EETQ_REQUIRE(out_buf, "spec_sample_accept: out_tokens is null");
    EETQ_REQUIRE(s_idx, "spec_sample_accept: column is null");
    EETQ_REQUIRE(s_pos, "spec_sample_accept: position is null");
    EETQ_REQUIRE(s_limit, "spec_sample_accept: limit is null");
    EETQ_REQUIRE(s_tok, "spec_sample_accept: next_token is null");
    EETQ_REQUIRE(hist, "spec_sample_accept: hist is null");
    EETQ_REQUIRE(stats, "spec_sample_accept: stats is null");
    EETQ_REQUIRE(params, "spec_sample_accept: params is null");
    EETQ_REQUIRE(workspace, "spec_sample_accept: workspace is null");
    EETQ_REQUIRE(k >= 1 && k <= kMaxDraft, "spec_sample_accept: k must lie in 1 .. 15");
    EETQ_REQUIRE(vocab > 0, "spec_sample_accept: vocab must be positive");
    EETQ_REQUIRE(batch > 0, "spec_sample_accept: batch must be positive");
    EETQ_REQUIRE((long)batch * (k + 1) < (1L << 24),
                 "spec_sample_accept: batch * (k + 1) must be below 2^24 (the workgroups are counted in 24 bits)");
    EETQ_REQUIRE(stride_t >= vocab, "spec_sample_accept: the logits' position stride must be at least vocab");
    EETQ_REQUIRE(stride_b >= vocab, "spec_sample_accept: the logits' batch stride must be at least vocab");
    EETQ_REQUIRE(draft_stride >= k, "spec_sample_accept: the draft's row stride must be at least k");
    EETQ_REQUIRE(out_cols > 0 && out_stride >= out_cols, "spec_sample_accept: out_stride must be at least out_cols, out_cols positive");
    EETQ_REQUIRE(hist_cols > 0 && hist_stride >= hist_cols,
                 "spec_sample_accept: the history's row stride must be at least cols, cols positive");
    EETQ_REQUIRE(tok_stride >= 1, "spec_sample_accept: next_token's row stride must be at least 1");
    EETQ_REQUIRE(!uniforms || uniforms_stride >= k + 1, "spec_sample_accept: the uniforms' row stride must be at least k + 1");
    EETQ_REQUIRE((uintptr_t)draft % 8 == 0 && (uintptr_t)out_buf % 8 == 0 && (uintptr_t)s_idx % 8 == 0 && (uintptr_t)s_pos % 8 == 0 &&
                     (uintptr_t)s_limit % 8 == 0 && (uintptr_t)s_tok % 8 == 0 && (uintptr_t)hist % 8 == 0 && (uintptr_t)stats % 8 == 0 &&
                     (uintptr_t)workspace % 8 == 0,
                 "spec_sample_accept: int64 pointers must be 8-byte aligned");
    EETQ_REQUIRE((uintptr_t)params % 8 == 0, "spec_sample_accept: params must be 8-byte aligned");
    EETQ_REQUIRE((uintptr_t)logits % 2 == 0, "spec_sample_accept: logits must be 2-byte aligned");
    spec_sample_accept_kernel<<<batch * (k + 1), kThreads, 0, stream>>>(
        logits, stride_b, stride_t, vocab, batch, k, draft, draft_stride, out_buf, out_stride, out_cols, s_idx, s_pos, s_limit, s_tok,
        tok_stride, hist, hist_stride, hist_cols, stats, static_cast<const SampleParams*>(params), done, uniforms, uniforms_stride,
        workspace);
    return check_hip(hipGetLastError(), "spec_sample_accept_kernel launch");
}

}  // namespace eetq

extern "C" {

int eetq_spec_sample_accept_f16(const void* logits, long stride_b, long stride_t, int vocab, int batch, int k, const int64_t* draft,
                                long draft_stride, int64_t* out_tokens, long out_stride, int out_cols, int64_t* column,
                                int64_t* position, const int64_t* limit, int64_t* next_token, long next_stride, int64_t* hist,
                                long hist_stride, int hist_cols, int64_t* stats, const void* params, int32_t* done,
                                const float* uniforms, long uniforms_stride, int64_t* workspace, void* stream)
{
    return eetq::launch_spec_sample_accept(static_cast<const eetq::f16*>(logits), stride_b, stride_t, vocab, batch, k, draft,
                                           draft_stride, out_tokens, out_stride, out_cols, column, position, limit, next_token,
                                           next_stride, hist, hist_stride, hist_cols, stats, params, done, uniforms, uniforms_stride,
                                           workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"
