"""Inputs and one float64 reference for the decode-attention kernels (eetq_decode_attention_f16, eetq_rope_decode_attention_f16).
A plain module for the tests (not a conftest), NumPy only, CPU only.  It shares no code with the kernels or with the other tests.

Three input families (every array is float16 unless said otherwise; caches are [B, Hkv, S, D], queries [B, H, D]):

  hot row   one key of a head is c * q with c chosen so that its scaled score beats every other score of the head by more
            than GAP_MIN = 200 natural-log units: exp(-200) is 0 in fp32 with or without denormals (the least fp32 denormal is
            exp(-103.3)), so every other weight is exactly 0, the hot weight exactly 1, and the answer is the hot row of V,
            bit for bit.  A skipped row, or a V row paired with the wrong K row, cannot hide in a tolerance.
  census    q = 0: every weight is 1 and the answer is the mean of small integers, exact in fp32 up to the final division.
            A row counted twice (which a hot row cannot show: 2v / 2 = v) or dropped moves the mean by many fp16 ulps.
  random    N(0, 1) everywhere and an aperiodic additive mask of -inf holes, zeros and finite ALiBi-like slopes.
"""
import numpy as np

GAP_MIN = 200.0      # what the tests assert
GAP_TARGET = 260.0   # what the generators aim at (fp16 rounding of c * q and of a rotation moves a score by well under 1)


def normal_f16(rng, shape):
    return rng.standard_normal(shape, dtype=np.float32).astype(np.float16)


def nonzero_normal_f16(rng, shape):
    """N(0, 1) without zeros: bit equality and value equality are then the same thing (-0 == +0 cannot blur it)."""
    v = normal_f16(rng, shape)
    v[v == 0] = np.float16(1.0)
    return v


def expand_heads(x, H):
    """[B, Hkv, ...] -> [B, H, ...]: query head h reads kv head h // (H / Hkv)."""
    return np.repeat(x, H // x.shape[1], axis=1)


def reference(q, k, v, sv, scale, mask=None):
    """float64 softmax(scale q k^T + mask) v over the first sv cache rows of the fp16 inputs.  q [B, H, D]; k, v [B, Hkv, S, D];
    mask [B or 1, >= S] additive or None.  A query with no attendable row (sv == 0, or every row at -inf) gives zeros."""
    B, H, D = q.shape
    out = np.zeros((B, H, D), dtype=np.float64)
    if sv <= 0:
        return out
    kk = expand_heads(np.asarray(k)[:, :, :sv], H).astype(np.float64)
    vv = expand_heads(np.asarray(v)[:, :, :sv], H).astype(np.float64)
    s = np.einsum("bhd,bhsd->bhs", np.asarray(q).astype(np.float64), kk) * float(scale)
    if mask is not None:
        m = np.asarray(mask).astype(np.float64)
        m = np.broadcast_to(m, (B, m.shape[1]))
        s = s + m[:, None, :sv]
    top = s.max(axis=-1, keepdims=True)
    alive = np.isfinite(top[..., 0])
    with np.errstate(invalid="ignore"):
        p = np.where(alive[..., None], np.exp(s - np.where(np.isfinite(top), top, 0.0)), 0.0)
    den = p.sum(axis=-1)
    num = np.einsum("bhs,bhsd->bhd", p, vv)
    out[alive] = num[alive] / den[alive][:, None]
    return out


def scores(q, k, scale):
    """float64 scale * q . k for every cache row: [B, H, S]."""
    kk = expand_heads(np.asarray(k), q.shape[1]).astype(np.float64)
    return np.einsum("bhd,bhsd->bhs", np.asarray(q).astype(np.float64), kk) * float(scale)


# ---- hot row -------------------------------------------------------------------------------------------------------------

def hot_keys(q, scale, target=GAP_TARGET):
    """k = fp16(c q), c per (b, h) such that scale * q . k is about `target`."""
    q64 = np.asarray(q).astype(np.float64)
    c = target / (float(scale) * (q64 * q64).sum(-1))
    return (q64 * c[..., None]).astype(np.float16)


def hot_base(B, H, S, D, seed):
    """q [B, H, D], k, v [B, H, S, D] (every head its own rows), v without zeros, and the hot keys of the two strengths the
    variants use: `hot` beats the random rows by GAP_TARGET, `hotter` beats `hot` by another GAP_TARGET."""
    rng = np.random.default_rng(seed)
    q = normal_f16(rng, (B, H, D))
    k = normal_f16(rng, (B, H, S, D))
    v = nonzero_normal_f16(rng, (B, H, S, D))
    scale = D ** -0.5
    return dict(q=q, k=k, v=v, scale=scale, hot=hot_keys(q, scale), hotter=hot_keys(q, scale, 2 * GAP_TARGET))


def hot_gap(q, k, hot, scale):
    """Least margin, over the heads, of the hot key's float64 score over EVERY row of k (so it holds wherever the hot key
    replaces a row)."""
    q64 = np.asarray(q).astype(np.float64)
    s_hot = (q64 * np.asarray(hot).astype(np.float64)).sum(-1) * float(scale)
    return float((s_hot - scores(q, k, scale).max(-1)).min())


def sweep(n_valid, heads, launch):
    """The hot position of each of `heads` (b, h) pairs in launch `launch` of a sweep over [0, n_valid): consecutive
    positions, all different within a launch (while heads <= n_valid); the last launch wraps around."""
    return (launch * heads + np.arange(heads)) % n_valid


def sweep_launches(n_valid, heads):
    return (n_valid + heads - 1) // heads


# ---- census --------------------------------------------------------------------------------------------------------------

def census_values(B, Hkv, S, D, seed):
    """V: nonzero integers in [-8, 8], |V[s, d]| = 8 for at least one d of every row.  K: N(0, 1) (q = 0 makes it irrelevant)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 9, size=(B, Hkv, S, D)) * rng.choice([-1, 1], size=(B, Hkv, S, D))
    d8 = rng.integers(0, D, size=(B, Hkv, S, 1))
    np.put_along_axis(v, d8, 8 * rng.choice([-1, 1], size=d8.shape), axis=-1)
    return v.astype(np.float16), normal_f16(rng, (B, Hkv, S, D))


def fp16_ulp(x):
    """Spacing of float16 at |x| (float64 in, float64 out); 2^-24 in the subnormal range and at 0."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    _, ex = np.frexp(a)                      # a = m 2^ex, m in [0.5, 1)
    e = np.maximum(ex - 1, -14)
    return np.where(a == 0, 2.0 ** -24, np.ldexp(1.0, e - 10))


def census_shift_ulps(v, sv):
    """By how many fp16 ulps (of the true mean) the worst-placed single row moves its best channel when it is dropped and
    when it is counted twice: (drop, double), the minimum over heads and rows of the maximum over channels.  sv == 1 has
    no `double` figure: counting the only row twice gives 2v / 2, the same answer -- softmax cannot show it."""
    x = np.asarray(v)[:, :, :sv].astype(np.float64)
    mean = x.mean(axis=2, keepdims=True)
    ulp = fp16_ulp(mean)
    if sv == 1:
        return float((np.abs(x) / ulp).max(-1).min()), None   # dropping the only row leaves zeros
    drop = np.abs(mean - x) / (sv - 1) / ulp
    dbl = np.abs(x - mean) / (sv + 1) / ulp
    return float(drop.max(-1).min()), float(dbl.max(-1).min())


# ---- random, with finite masks ---------------------------------------------------------------------------------------------

def random_case(B, H, Hkv, S, D, seed):
    rng = np.random.default_rng(seed)
    return dict(q=normal_f16(rng, (B, H, D)), k=normal_f16(rng, (B, Hkv, S, D)), v=normal_f16(rng, (B, Hkv, S, D)),
                scale=D ** -0.5)


def random_mask(B, width, seed):
    """[B, width]: an ALiBi-like slope per batch row (finite, negative, growing with the distance from the last column),
    15 % of the columns knocked out with -inf and 30 % set to 0, at independent random places."""
    rng = np.random.default_rng(seed)
    slope = 2.0 ** -(3.0 + rng.integers(0, 4, size=(B, 1)))
    m = -slope * (width - 1 - np.arange(width))[None, :]
    u = rng.random((B, width))
    m[u < 0.15] = -np.inf
    m[(u >= 0.15) & (u < 0.45)] = 0.0
    return m.astype(np.float16)


# ---- the new token of the one-launch form ----------------------------------------------------------------------------------

def rope_table(D, rows):
    """cos | sin table [rows, D] of the NeoX rotation, base 10000, float16."""
    inv = 1.0 / (10000.0 ** (np.arange(0, D, 2, dtype=np.float64) / D))
    fr = np.arange(rows, dtype=np.float64)[:, None] * inv[None, :]
    return np.concatenate([np.cos(fr), np.sin(fr)], axis=-1).astype(np.float16)


def rope_neox_f16(x, table, positions):
    """NeoX rotation of x [B, heads, D] by positions [B], in float16 with a rounding after every multiply and add (NumPy's
    float16 arithmetic does exactly that): channel d < D/2 pairs with d + D/2."""
    D = x.shape[-1]
    row = np.asarray(table)[np.asarray(positions)]
    c, s = row[:, None, : D // 2], row[:, None, D // 2:]
    lo, hi = np.asarray(x)[..., : D // 2], np.asarray(x)[..., D // 2:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=-1).astype(np.float16)


def new_token_hot(B, H, S, D, seed, table_rows=2048):
    """A full random cache and a new token whose key is c * q BEFORE the rotation: both are rotated by the same position, so
    the rotated pair still scores about GAP_TARGET.  v_new has no zeros."""
    rng = np.random.default_rng(seed)
    q = normal_f16(rng, (B, H, D))
    scale = D ** -0.5
    return dict(q=q, k_new=hot_keys(q, scale), v_new=nonzero_normal_f16(rng, (B, H, D)), kc=normal_f16(rng, (B, H, S, D)),
                vc=nonzero_normal_f16(rng, (B, H, S, D)), pos=rng.integers(1, table_rows, size=B).astype(np.int64),
                table=rope_table(D, table_rows), scale=scale)


def new_token_gap(case):
    """Least margin of the rotated new key's float64 score over every cache row, for the rotated query."""
    qr = rope_neox_f16(case["q"], case["table"], case["pos"])
    kr = rope_neox_f16(case["k_new"], case["table"], case["pos"])
    return hot_gap(qr, case["kc"], kr, case["scale"])
