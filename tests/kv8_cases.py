"""Inputs and references for the int8 KV cache (eetq_decode_attention_i8kv_f16, eetq_rope_decode_attention_i8kv_f16,
eetq_rotary_neox_kvcache_prefill_i8_f16).  A plain module for the tests (not a conftest), NumPy only, CPU only; it restates the
row quantiser of include/eetq_amd.h ("The int8 KV cache") and its inverse, shares no code with the kernels, and takes
everything else from attn_cases.

One cache ROW is the D fp16 values of one (batch row, kv head, position):
    amax = max |x_d|                                   exact
    s    = fp16(fp32(amax) * (1.0f / 127.0f))          one fp32 multiply, round to nearest even
    q_d  = clamp(round_half_away(fp32(x_d) / fp32(s)), -127, 127)      IEEE fp32 division; s == 0 -> q = 0
Attention is over the dequantised rows s * q taken as exact reals: float64 holds them exactly (11 x 8 significant bits).
"""
import numpy as np

import attn_cases as ac

INV127 = np.float32(1.0) / np.float32(127.0)


def quantize_rows(x):
    """x float16 [..., D] -> (q int8 [..., D], s float16 [...])."""
    x32 = np.asarray(x, dtype=np.float16).astype(np.float32)
    amax = np.abs(x32).max(axis=-1)
    s = (amax * INV127).astype(np.float16)          # float32 product, then round to nearest even
    s32 = s.astype(np.float32)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (x32 / s32).astype(np.float64)          # IEEE float32 quotient, held exactly
    r = np.where(s32 == 0, 0.0, r)
    q = np.sign(r) * np.floor(np.abs(r) + 0.5)      # half away from zero, exact in float64
    return np.clip(q, -127, 127).astype(np.int8), s


def dequantize_rows(q, s):
    """float64 s * q, exact."""
    return np.asarray(q).astype(np.float64) * np.asarray(s).astype(np.float64)[..., None]


def scale_pairs(ks, vs):
    """[..., 2] float16 = (k scale, v scale): the scale tensor of a cache."""
    return np.stack([np.asarray(ks, dtype=np.float16), np.asarray(vs, dtype=np.float16)], axis=-1)


def quantize_cache(k, v):
    """fp16 K, V [B, Hkv, S, D] -> dict(k8, v8 int8, scales float16 [B, Hkv, S, 2], kd, vd float64 dequantised)."""
    k8, ks = quantize_rows(k)
    v8, vs = quantize_rows(v)
    return dict(k8=k8, v8=v8, scales=scale_pairs(ks, vs), kd=dequantize_rows(k8, ks), vd=dequantize_rows(v8, vs))


def hot_value(v8, vs):
    """What a row that holds all the weight returns: fp16(vs * v8), one rounding of the exact product."""
    return dequantize_rows(v8, vs).astype(np.float16)


def census_scales(S):
    """V scales cycling 0.5, 1, 2 by row: [S] float16."""
    return np.array([0.5, 1.0, 2.0], dtype=np.float16)[np.arange(S) % 3]
