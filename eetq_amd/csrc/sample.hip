// Sampling decode hand-over (extension for the HIP-graph decoder, utils/graph_decoder.py): temperature, top-k,
// top-p and the draw of one token per batch row of fp16 logits (sample_row.hpp), then the bookkeeping of greedy_handover_kernel
// (norm_rope.hip) -- one launch, no sort.
// One workgroup per row; the row that finishes last advances *position and *column (a ticket in the upper bits of *position),
// so every row has read *column before anyone advances it.
#include "sample_row.hpp"

namespace eetq {

namespace {

__global__ __launch_bounds__(kThreads) void sample_handover_kernel(const f16* __restrict__ logits, long row_stride, int vocab, int batch,
                                                                   int64_t* __restrict__ out_buf, long out_stride, int out_cols,
                                                                   int64_t* s_idx, int64_t* __restrict__ s_tok,
                                                                   int64_t* s_pos, const SampleParams* __restrict__ params,
                                                                   int* __restrict__ done, const float* __restrict__ uniforms)
{
    __shared__ Lds     s;
    const int          tid = threadIdx.x, b = blockIdx.x;   // one workgroup per row
    const int64_t      col = __hip_atomic_load(s_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const SampleParams p   = *params;
    const bool         sampled = p.temperature > 0.f;   // 0, negative and NaN select greedy
    int64_t            tok;
    if (done && done[b] != 0) {
        tok = (int64_t)p.pad_token;
    } else {
        const f16* row = logits + (long)b * row_stride;
        if (sampled) {
            u32 m_u;
            if (uniforms) {
                const float u = uniforms[b];
                m_u           = !(u > 0.f) ? 0u : u >= 1.f ? 0xFFFFFFu : (u32)(u * 16777216.f);
            } else {
                m_u = philox4x32_10((u32)(u64)col, (u32)((u64)col >> 32), (u32)b, 0u, (u32)p.seed, (u32)(p.seed >> 32)).x[0] >> 8;
            }
            tok = sample_row(row, vocab, p.temperature, p.top_p, p.top_k, m_u, s);
        } else {
            tok = greedy_row(row, vocab, s);
        }
    }
    if (tid == 0) {
        if (col >= 0 && col < out_cols) out_buf[b * out_stride + col] = tok;
        s_tok[b] = tok;
        if (done && p.eos_token >= 0 && tok == (int64_t)p.eos_token) done[b] = 1;
        // The advance waits for the last row: every workgroup has read *column (above, before this release) by the time it
        // takes a ticket.  The ticket lives in bits 40.. of *position itself for the length of the launch -- no workspace, no
        // state between launches, nothing shared with a launch on other counters; the last row takes the tickets out again.
        u64* pos = reinterpret_cast<u64*>(s_pos);
        const u64 old = __hip_atomic_fetch_add(pos, 1ull << kTicketShift, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        // (biased by 2^39, so that a negative position, which the greedy kernel tolerates, counts from 0 as well)
        if ((((old + (1ull << (kTicketShift - 1))) >> kTicketShift) & 0xFFFFFFull) == (u64)(batch - 1)) {
            __hip_atomic_fetch_add(pos, 1ull - ((u64)batch << kTicketShift), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(s_idx, col + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

int launch_sample_handover(const f16* logits, long row_stride, int vocab, int batch, int64_t* out_buf, long out_stride, int out_cols,
                           int64_t* s_idx, int64_t* s_tok, int64_t* s_pos, const void* params, int* done, const float* uniforms,
                           hipStream_t stream)
{
    EETQ_REQUIRE(logits, "sample_handover: logits is null");
    EETQ_REQUIRE(out_buf, "sample_handover: out_tokens is null");
    EETQ_REQUIRE(s_idx, "sample_handover: column is null");
    EETQ_REQUIRE(s_tok, "sample_handover: next_token is null");
    EETQ_REQUIRE(s_pos, "sample_handover: position is null");
    EETQ_REQUIRE(params, "sample_handover: params is null");
    EETQ_REQUIRE(vocab > 0, "sample_handover: vocab must be positive");
    EETQ_REQUIRE(batch >= 0, "sample_handover: batch must not be negative");
    EETQ_REQUIRE(row_stride >= vocab, "sample_handover: row_stride must be at least vocab");
    EETQ_REQUIRE(out_cols > 0, "sample_handover: out_cols must be positive");
    EETQ_REQUIRE(out_stride >= out_cols, "sample_handover: out_stride must be at least out_cols");
    EETQ_REQUIRE((uintptr_t)params % 8 == 0, "sample_handover: params must be 8-byte aligned");
    EETQ_REQUIRE(batch < (1 << 24), "sample_handover: batch must be below 2^24 (the rows are counted in 24 bits)");
    if (batch == 0) return EETQ_OK;
    sample_handover_kernel<<<batch, kThreads, 0, stream>>>(logits, row_stride, vocab, batch, out_buf, out_stride, out_cols, s_idx, s_tok, s_pos,
                                                       static_cast<const SampleParams*>(params), done, uniforms);
    return check_hip(hipGetLastError(), "sample_handover_kernel launch");
}

}  // namespace eetq
