// Input gradient of the W8A16 projection, gfx950: dx[M][K] = fp16( sum_n dy[M][n] * fp16(q[k][n] * s[n]) ), i.e. the
// `grad @ W_deq^T` of the reference's backward (python/eetq/modules/qlinear.py:80-94) without materialising W_deq.
//
// Structure:
//   * workgroup tile 128 rows of M x 128 columns of K, reduction over N in 64-wide steps; 4 waves = 2 row halves x 2 K halves,
//     a wave owns 64 rows x 64 k: 2 x 2 blocks of v_mfma_f32_32x32x16_f16, 64 fp32 accumulators per lane, no cross-wave sum;
//   * the weight is the A operand (A[k][n]) and dy the B operand (B[n][m]): an accumulator lane then holds 4 consecutive k of
//     one row m, written as 8 bytes into a row-major fp16 image of the tile and stored with whole-row 16-byte stores;
//   * the native layout gives a lane 16 k of ONE column n, the A operand wants 8 n of one k: each wave loads one 16-column
//     group of the step's 128 k x 64 n block (two 1 KiB tiles), dequantises it ONCE for the workgroup (dequant_16, the
//     forward's exact fp16(q * s)) and writes an fp16 image with rows = n, 256-byte rows of k; ds_read_b64_tr_b16 reads it
//     back transposed (4 consecutive n of one k per lane, two reads per fragment).  Image swizzle: chunk ^ ((row & 3) << 2 | (row >> 2) & 3),
//     conflict-free for the transposed reads (four rows x four chunks of a half-wave land on 64 distinct banks);
//   * dy is staged in registers -> LDS as 128-byte rows, 16-byte chunks XOR-swizzled by (row >> 1) & 7 (the forward's
//     activation image: ds_read_b128 of 32 rows at one n offset is conflict-free);
//   * two LDS stages (64 KiB, two workgroups per CU) and two register sets of global loads: the loads of step s + 2 are in
//     flight while step s computes; one barrier per step;
//   * tails: k columns beyond K (K % 128 == 64) are computed from a clamped tile and never stored; 16-column groups beyond
//     N write zeros into the weight image and dy chunks beyond N are zero, so ragged N adds exact zeros; rows beyond M read
//     row M - 1 and are not stored.  One pass over N per tile, no atomics: the result bits do not depend on the launch.
// The kernel itself is the BITS = 8 instantiation of gemm_t_kernel.hpp (shared with gemm_t_int4.hip and
// moe_gemm_t_int4.hip, whose producer reads int4 tiles).
#include "gemm_t_kernel.hpp"

namespace eetq {

int launch_gemm_t(const f16* dy, const uint8_t* w, const f16* scales, f16* dx, int M, int N, int K, hipStream_t stream)
{
    using namespace gemm_t;
    const int tiles = ((M + BM - 1) / BM) * ((K + BK - 1) / BK);
    launch_kernel(gemm_t_kernel<false, 8>, dim3(tiles), dim3(256), SMEM_BYTES, stream, dy, w, scales, dx, M, N, K, (const int*)nullptr,
                  (const int*)nullptr, 0);
    return check_hip(hipGetLastError(), "gemm_t_kernel launch");
}

int launch_moe_gemm_t(const f16* dy, const uint8_t* w, const f16* scales, const int* offsets, const int* active, f16* dx, int S,
                      int E, int N, int K, hipStream_t stream)
{
    using namespace gemm_t;
    const int A = S < E ? S : E;
    const int R = S / BM + A;
    launch_kernel(gemm_t_kernel<true, 8>, dim3(R * ((K + BK - 1) / BK)), dim3(256), SMEM_BYTES, stream, dy, w, scales, dx, A, N, K,
                  offsets, active, R);
    return check_hip(hipGetLastError(), "gemm_t_kernel<grouped> launch");
}

}  // namespace eetq
