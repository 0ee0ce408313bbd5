// The int8 KV-cache row format: one row = the D fp16 values of one (batch row, kv head, position), quantised
// symmetrically with a scale of its own.
//   amax = max |x_d|                                   (exact)
//   s    = fp16(fp32(amax) * (1.0f / 127.0f))           one fp32 multiply, round to nearest even
//   q_d  = clamp(round_half_away(fp32(x_d) / fp32(s)), -127, 127)   IEEE fp32 divide (the Makefile asks for it); s == 0 -> 0
// bytes are plain two's complement; -128 is never written.  Shared by the writers (norm_rope.hip, attn_decode.hip) so that
// every path to a cache row produces the same bits, and by the reader for the way back.
#pragma once
#include "common.hpp"

namespace eetq {

__device__ __forceinline__ float kv8_abs_max8(const f16x8& x)
{
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf((float)x[i]));
    return a;
}

__device__ __forceinline__ f16 kv8_scale(float amax) { return (f16)(amax * (1.0f / 127.0f)); }

// this lane's 8 channels -> 8 bytes (channel i in byte i)
__device__ __forceinline__ u32x2 kv8_quant8(const f16x8& x, f16 scale)
{
    const float s = (float)scale;
    u32         w[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float r = s != 0.f ? __builtin_roundf((float)x[i] / s) : 0.f;
        r       = fminf(fmaxf(r, -127.f), 127.f);
        w[i >> 2] |= ((u32)(int)r & 0xffu) << (8 * (i & 3));
    }
    return u32x2{w[0], w[1]};
}

// 8 bytes -> the exact integers as fp16 pairs (0, 1) (2, 3) (4, 5) (6, 7): the biased-byte trick of the weight kernels
// (dequant_dword) with one xor per dword to get from two's complement to q + 128
__device__ __forceinline__ void kv8_unpack8(const u32x2& w, f16x2 (&h)[4])
{
    const u32   c64  = 0x64646464u;
    const f16x2 bias = {(f16)1152.0f, (f16)1152.0f};
    const u32   x0 = w.x ^ 0x80808080u, x1 = w.y ^ 0x80808080u;
    h[0] = as_f16x2(__builtin_amdgcn_perm(x0, c64, 0x00050004u)) - bias;  // bytes [b0, 0x64, b1, 0x64]
    h[1] = as_f16x2(__builtin_amdgcn_perm(x0, c64, 0x00070006u)) - bias;  // bytes [b2, 0x64, b3, 0x64]
    h[2] = as_f16x2(__builtin_amdgcn_perm(x1, c64, 0x00050004u)) - bias;
    h[3] = as_f16x2(__builtin_amdgcn_perm(x1, c64, 0x00070006u)) - bias;
}

// the rules every attention entry over an int8 cache shares (attn_decode.hip, attn_prefill.hip): cache strides {k_b, k_h, k_pos,
// v_b, v_h, v_pos} in bytes (8-byte loads), scale strides in fp16 elements (one dword per row)
inline int check_i8_cache(const void* kc, const void* vc, const void* scales, int S, const long* cst, const long* sst)
{
    for (int i = 0; i < 6; ++i) EETQ_REQUIRE(cst[i] % 8 == 0, "int8 cache strides must be multiples of 8 bytes (8-byte accesses)");
    EETQ_REQUIRE(((uintptr_t)kc | (uintptr_t)vc) % 8 == 0, "the int8 caches must be 8-byte aligned");
    for (int i = 0; i < 3; ++i)
        EETQ_REQUIRE(sst[i] % 2 == 0, "the scale strides must be multiples of 2 elements (one dword per row: k scale, v scale)");
    EETQ_REQUIRE((uintptr_t)scales % 4 == 0, "the scales must be 4-byte aligned");
    EETQ_REQUIRE(cst[2] > 0 && cst[5] > 0 && sst[2] > 0 && ((long)S + 4096) * cst[2] < (1L << 31) &&
                     ((long)S + 4096) * cst[5] < (1L << 31) && ((long)S + 4096) * sst[2] * 2 < (1L << 31),
                 "one head's cache rows must span less than 2 GiB");
    return EETQ_OK;
}

}  // namespace eetq
