// The fp8 KV-cache row format: one row = the D fp16 values of one (batch row, kv head, position), each held as
// one byte of OCP e4m3fn (bias 7, no infinities, maximum 448, subnormals down to 2^-9).  The scale is per kv head, not per row:
// scales fp32 [kv_heads][2] = (k scale, v scale), positive, finite, shared by every batch row and position.
//   byte = e4m3_rne(clamp(fp32(x) / s, -448, 448))     IEEE fp32 divide (the Makefile asks for it), round to nearest even,
//                                                      subnormal results included; the clamp comes first, so the convert
//                                                      instruction never sees a value it would have to saturate
// Non-finite inputs are outside the contract.  Every e4m3 value is exact in fp16 and in fp32: the way back is a plain convert.
// Shared by the writers (norm_rope.hip, attn_decode.hip) so that every path to a cache row produces the same bits, and by the
// reader.  gfx950 converts in hardware: v_cvt_pk_fp8_f32 (two floats -> two bytes of a dword half), v_cvt_pk_f32_fp8 and
// v_cvt_scalef32_pk_f16_fp8 (two bytes -> two floats / an fp16 pair, here with the scale operand 1.0).
#pragma once
#include "common.hpp"

namespace eetq {

typedef float f32x2_f8 __attribute__((ext_vector_type(2)));

// this lane's 8 channels -> 8 bytes (channel i in byte i); s: the head's scale
__device__ __forceinline__ u32x2 kvf8_quant8(const f16x8& x, float s)
{
    float r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = fminf(fmaxf((float)x[i] / s, -448.f), 448.f);
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(r[0], r[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(r[2], r[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(r[4], r[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(r[6], r[7], w1, true);
    return u32x2{(u32)w0, (u32)w1};
}

// 8 bytes -> the exact values as fp16 pairs (0, 1) (2, 3) (4, 5) (6, 7), ready for v_dot2_f32_f16
__device__ __forceinline__ void kvf8_unpack8_f16(const u32x2& w, f16x2 (&h)[4])
{
    h[0] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.0f, false);
    h[1] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.x, 1.0f, true);
    h[2] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.0f, false);
    h[3] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w.y, 1.0f, true);
}

// 8 bytes -> the exact values in fp32
__device__ __forceinline__ void kvf8_unpack8_f32(const u32x2& w, float (&f)[8])
{
    const f32x2_f8 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
    const f32x2_f8 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
    f[0] = a.x, f[1] = a.y, f[2] = b.x, f[3] = b.y, f[4] = c.x, f[5] = c.y, f[6] = d.x, f[7] = d.y;
}

// the rules every entry over an fp8 cache shares: cache strides {k_b, k_h, k_pos, v_b, v_h, v_pos} in bytes (8-byte accesses)
inline int check_f8_cache(const void* kc, const void* vc, const void* scales, int S, const long* cst)
{
    EETQ_REQUIRE(scales, "null pointer");
    for (int i = 0; i < 6; ++i) EETQ_REQUIRE(cst[i] % 8 == 0, "fp8 cache strides must be multiples of 8 bytes (8-byte accesses)");
    EETQ_REQUIRE(((uintptr_t)kc | (uintptr_t)vc) % 8 == 0, "the fp8 caches must be 8-byte aligned");
    EETQ_REQUIRE((uintptr_t)scales % 4 == 0, "the fp8 scales must be 4-byte aligned");
    EETQ_REQUIRE(cst[2] > 0 && cst[5] > 0 && ((long)S + 4096) * cst[2] < (1L << 31) && ((long)S + 4096) * cst[5] < (1L << 31),
                 "one head's cache rows must span less than 2 GiB");
    return EETQ_OK;
}

}  // namespace eetq
