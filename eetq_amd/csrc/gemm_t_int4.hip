// Input gradient of the W4A16 projection, gfx950: dx[M][K] = fp16( sum_n dy[M][n] * fp16(q[k][n] * s[n]) ), q in -8..7 read
// straight from the gfx950 int4 tiles -- no expansion to int8 tiles, no K x N fp16 copy of the weight.
//
// The kernel is gemm_t_kernel.hpp's tile (see gemm_t.hip's header) with BITS = 4: BM = BK = 128, BN = 64, 4 waves,
// v_mfma_f32_32x32x16_f16, the same fp16 weight image and swizzle, dy stage, two-stage pipeline and row-store epilogue, hence the
// same accumulation order -- the result bits equal eetq_w8a16_gemm_t on the same integers held as int8 tiles.  Only the weight
// producer differs:
//   * layout: 1 KiB tiles of 16 columns x 128 k, ordered [n / 16][k / 128]; lane ((k >> 5) & 3) * 16 + (n & 15) holds 32 k of one
//     column in 16 bytes; dword d holds k = 8 d .. 8 d + 7 as nibbles q + 8 at positions [0, 4, 1, 5, 2, 6, 3, 7];
//   * per step a wave loads ONE tile (its 16-column group x the output tile's 128 k): one u32x4 per lane instead of two;
//   * two dequant_16_i4_perm calls on dwords (0, 1) and (2, 3): the values of dequant_16_i4 (gemm_kernel.hpp, the forward's exact
//     fp16(q) * s with one rounding) with the nibbles unpacked through v_perm_b32 (28 instead of 44 VALU instructions per lane and
//     step; DESIGN.md 4.9 has both measured);
//   * the 32 fp16 go to image row n = 16 wave + (lane & 15), chunks 4 (lane >> 4) + 0..3, as four 16-byte LDS stores;
//   * K % 128 == 0 is a precondition of the layout: no K tail.  Ragged N (a 16-column group beyond N stores zeros, dy chunks beyond
//     N load as zeros) and ragged M (rows clamped on read, not stored) are the template's.
// LDS banks of those stores, by the rule for ds_write_b128 (eight groups of 8 consecutive lanes, bank = (addr / 4) mod 32): a row
// is 256 bytes, so the bank depends on the physical chunk (ch ^ key(row)) mod 8 alone, key = (row & 3) << 2 | (row >> 2) & 3.  One
// logical chunk over 16 consecutive rows visits all 16 physical chunks once (the key is a bijection of row mod 16) = every one of
// the 64 dword columns of the row once; within one 8-lane group the 8 rows reach only 4 distinct values of key mod 8 (row bit 1
// lands in key bit 3), i.e. two rows per 4-bank set: the store takes 16 LDS-array cycles against the ~13 its data transfer costs
// anyway.  The int8 producer writes the same rows through the same key, so this is unchanged from gemm_t.hip -- and changing the
// key would change the conflict-free transposed reads (16 per wave and step against these 4 stores).
#include "gemm_t_kernel.hpp"

namespace eetq {

int launch_gemm_t_i4(const f16* dy, const uint8_t* w, const f16* scales, f16* dx, int M, int N, int K, hipStream_t stream)
{
    using namespace gemm_t;
    const int tiles = ((M + BM - 1) / BM) * (K / BK);
    launch_kernel(gemm_t_kernel<false, 4>, dim3(tiles), dim3(256), SMEM_BYTES, stream, dy, w, scales, dx, M, N, K, (const int*)nullptr,
                  (const int*)nullptr, 0);
    return check_hip(hipGetLastError(), "gemm_t_kernel<int4> launch");
}

}  // namespace eetq
