// Input gradient of the routed W4A16 experts, gfx950: for every expert e of an int4 stack [E][K][N / 2], rows
// offsets[e] .. offsets[e + 1] - 1 of dx [S][K] = dy [S][N] . fp16(q_e s_e)^T, q in -8..7 read straight from the gfx950 int4 tiles --
// no expansion of the stack to int8 tiles, which is what training through int4 experts did not have before this kernel.
//
// The kernel is gemm_t_kernel.hpp's GROUPED = true, BITS = 4 instantiation: the grouped row map of gemm_t.hip's
// launch_moe_gemm_t (R = floor(S / 128) + min(S, E) row-tile slots x K / 128 column tiles, every wave finds its slot's expert from the
// active list with a wave scan, surplus slots exit before any load) in front of gemm_t_int4.hip's tile body (one 1 KiB int4 tile per
// wave and step, dequant_16_i4_perm, the shared fp16 weight image).  Expert e's tiles start e * K * N / 2 bytes into the stack and its
// scales at e * N; nothing else differs, so an expert's rows are eetq_w4a16_gemm_t's bits on those rows and that expert's weight, and
// eetq_w8a16_moe_gemm_t's bits on the same integers held as an int8 stack.  It is a translation unit of its own so that gemm_t.o and
// gemm_t_int4.o stay the objects they were.
#include "gemm_t_kernel.hpp"
#include "moe_gemm_kernel.hpp"

namespace eetq {

int launch_moe_gemm_t_i4(const f16* dy, const uint8_t* w, const f16* scales, const int* offsets, const int* active, f16* dx, int S,
                         int E, int N, int K, hipStream_t stream)
{
    using namespace gemm_t;
    const int A = S < E ? S : E;
    const int R = S / BM + A;
    launch_kernel(gemm_t_kernel<true, 4>, dim3(R * (K / BK)), dim3(256), SMEM_BYTES, stream, dy, w, scales, dx, A, N, K, offsets, active,
                  R);
    return check_hip(hipGetLastError(), "gemm_t_kernel<grouped, int4> launch");
}

}  // namespace eetq

using namespace eetq;

extern "C" {

int eetq_w4a16_moe_gemm_t(const void* dy, const int8_t* w_packed_i4, const void* scales, const int* offsets, const int* active,
                          void* dx, int T, int k, int E, int N, int K, void* stream)
{
    EETQ_REQUIRE(dy && w_packed_i4 && scales && offsets && active && dx, "eetq_w4a16_moe_gemm_t: null pointer");
    EETQ_REQUIRE(E >= 1 && E <= kMoeMaxExperts, "eetq_w4a16_moe_gemm_t: E must be in [1, 1024]");
    EETQ_REQUIRE(k >= 1 && k <= E, "eetq_w4a16_moe_gemm_t: k must be in [1, E]");
    EETQ_REQUIRE(T >= 1 && (long long)T * k <= (1ll << 30), "eetq_w4a16_moe_gemm_t: T must be >= 1 and T * k <= 2^30");
    EETQ_REQUIRE(N >= 16 && N % 16 == 0 && K >= 128 && K % 128 == 0,
                 "eetq_w4a16_moe_gemm_t: the gfx950 int4 layout needs K % 128 == 0 and N % 16 == 0");
    EETQ_REQUIRE((long long)T * k * (N > K ? N : K) < (1ll << 40) && (long long)E * K * N / 2 < (1ll << 40) &&
                     ((long long)T * k / 128 + E) * (K / 128) < (1ll << 31),
                 "eetq_w4a16_moe_gemm_t: gradient or weight stack too large");
    EETQ_REQUIRE(aligned16(dy) && aligned16(w_packed_i4) && aligned16(dx),
                 "eetq_w4a16_moe_gemm_t: dy, weight and dx must be 16-byte aligned");
    return launch_moe_gemm_t_i4(static_cast<const f16*>(dy), reinterpret_cast<const uint8_t*>(w_packed_i4),
                                static_cast<const f16*>(scales), offsets, active, static_cast<f16*>(dx), T * k, E, N, K,
                                static_cast<hipStream_t>(stream));
}

}  // extern "C"
