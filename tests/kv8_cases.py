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


# ---- edge rows: inputs on which a quantiser that is subtly wrong differs from `quantize_rows` -------------------------------
U = 2.0 ** -24                                   # the least fp16 subnormal
TIE_EXPONENTS = (-7, 0)
TINY_N = (1, 63, 64, 127, 190, 191, 255, 1023)   # amax = n U: scale bits 0, 0, 1, 1, 1, 2, 2, 8


def _no_negative_zero(x):
    x = np.asarray(x, dtype=np.float16)
    x[x == 0] = 0                                # -0 -> +0: the identity rotation and a bit comparison then agree
    return x


def tie_rows(D):
    """For e in TIE_EXPONENTS and both signs sg: channel 0 = sg 127 2^e (scale 2^e exactly), channel c >= 1 holds
    sg (-1)^k (k + 0.5) 2^e, k running through 0..126 over as many rows as that takes (one at D = 128, three at D = 64, the
    last one wrapping round): every element is an exact tie, every k occurs with both signs.  Round-to-even differs from
    half-away at every even k."""
    per = D - 1
    n = -(-127 // per)
    rows = []
    for e in TIE_EXPONENTS:
        for sg in (1.0, -1.0):
            for i in range(n):
                k = (i * per + np.arange(per)) % 127
                row = np.empty(D, dtype=np.float64)
                row[0] = sg * 127.0
                row[1:] = sg * np.where(k % 2 == 0, 1.0, -1.0) * (k + 0.5)
                rows.append(row * 2.0 ** e)
    return np.array(rows).astype(np.float16)


def tiny_rows(D, seed=24):
    """amax = n U for n in TINY_N at channel 0 (signs alternating by row); channel 1 = (n // 2) U, channel 2 = U, the others
    random multiples of U no larger than amax, of both signs.  All of it is fp16-subnormal."""
    rng = np.random.default_rng(seed)
    rows = []
    for i, n in enumerate(TINY_N):
        m = rng.integers(0, n + 1, size=D) * rng.choice([-1, 1], size=D)
        m[0], m[1], m[2] = (n if i % 2 == 0 else -n), n // 2, 1
        rows.append(m * U)
    return _no_negative_zero(np.array(rows))


def extreme_rows(D):
    """amax = -65504 (scale 516): 258 and -258 are exact halves (-> 1, -1), 65504 -> 127; further exact halves 258 + 516 j of
    alternating sign, zeros elsewhere."""
    row = np.zeros(D, dtype=np.float64)
    row[:4] = [-65504.0, 258.0, -258.0, 65504.0]
    for j in range(1, 8):                        # 258 + 516 j <= 3870: even integers below 4096 are fp16 values
        row[3 + j] = (258.0 + 516.0 * j) * (1 if j % 2 else -1)
    return row[None].astype(np.float16)


def sweep_rows(D, seed=7):
    """D rows: row c has its maximum, fp16(1 + c / D) with the sign alternating, at channel c; every other channel is drawn
    from N(0, 0.2) and clipped to |x| <= 0.5.  The D scales differ pairwise, so a reduction that misses a lane gives a
    wrong scale in the row whose maximum sits there."""
    rng = np.random.default_rng(seed)
    rows = np.clip(rng.standard_normal((D, D)) * 0.2, -0.5, 0.5)
    c = np.arange(D)
    rows[c, c] = (1.0 + c / D) * np.where(c % 2 == 0, 1.0, -1.0)
    return _no_negative_zero(rows)


def edge_rows(D):
    """{family: float16 [n, D]} in a fixed order: ties, tiny, extreme, sweep, zero.  What they must quantise to is whatever
    `quantize_rows` gives; the builders only choose inputs (tests/test_kv8_cpu.py pins what the GPU tests rely on)."""
    return dict(ties=tie_rows(D), tiny=tiny_rows(D), extreme=extreme_rows(D), sweep=sweep_rows(D),
                zero=np.zeros((1, D), dtype=np.float16))


def edge_rows_flat(D):
    """(rows float16 [R, D], {family: slice}) of `edge_rows`"""
    fam = edge_rows(D)
    where, at = {}, 0
    for name, r in fam.items():
        where[name] = slice(at, at + len(r))
        at += len(r)
    return np.concatenate(list(fam.values())), where


def identity_table(D, rows):
    """cos | sin table [rows, D] with cos = 1 and sin = 0: the rotation x 1 - y 0 is exact, K reaches the quantiser as built"""
    t = np.zeros((rows, D), dtype=np.float16)
    t[:, : D // 2] = 1
    return t
