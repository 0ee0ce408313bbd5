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


# ==== prompt ("prefill") attention: eetq_prefill_attention_f16 ================================================================
# Queries [B, T, H, D], caches [B, Hkv, S, D] with S = keys + PREFILL_PAD; query t attends rows s < keys and s <= t + koff.
# Every generator poisons the cache rows >= keys with NaN.  Four families:
#
#   staircase    every query of a kv-head group is the same vector and key row r is its hot key: out[t] == V[r] bit for bit
#                for every t with t + koff >= r; before that the hot key is future bait and the answer is an ordinary softmax.
#   pairing      distinct queries, key row pi(t) is the hot key of query t (pi(t) = t + koff, or drawn from [0, t + koff]):
#                out[t] == V[pi(t)] bit for bit for all t of ONE launch.
#   census       q = 0: out[t] is the mean of the small integers V[0 .. min(keys, t + koff + 1) - 1], within 1 fp16 ulp.
#   random       N(0, 1), optionally with a ramp that makes every 64-key block's maximum exceed the one before.

PREFILL_PAD = 11     # cache rows beyond `keys` (NaN)
PAIR_MARGIN = 20.0   # the pairing generator raises its target until the least gap is GAP_MIN + this


def poison_tail(x, keys):
    """rows >= keys of a cache [B, Hkv, S, D] set to NaN (in place); returns x"""
    x[:, :, keys:] = np.float16(np.nan)
    return x


def prefill_counts(T, keys, koff):
    """attendable rows of every query: min(keys, t + koff + 1), at least 0"""
    return np.clip(np.arange(T) + koff + 1, 0, keys)


def prefill_reference(q, k, v, keys, koff, scale):
    """float64 softmax over the rows s < keys and s <= t + koff of the fp16 inputs.  q [B, T, H, D]; k, v [B, Hkv, S, D].
    Returns (out, absmean), both [B, T, H, D]: absmean = sum p |v| / sum p, the scale of the random bound.  A query with no
    attendable row gives zeros (as `reference` does)."""
    B, T, H, D = q.shape
    kk = expand_heads(np.asarray(k)[:, :, :keys], H).astype(np.float64)
    vv = expand_heads(np.asarray(v)[:, :, :keys], H).astype(np.float64)
    s = np.matmul(np.asarray(q).astype(np.float64).transpose(0, 2, 1, 3), kk.transpose(0, 1, 3, 2)) * float(scale)   # [B, H, T, keys]
    allowed = np.arange(keys)[None, :] <= (np.arange(T)[:, None] + koff)
    s = np.where(allowed, s, -np.inf)
    top = s.max(axis=-1, keepdims=True)
    alive = np.isfinite(top)
    with np.errstate(invalid="ignore"):
        p = np.where(alive, np.exp(s - np.where(alive, top, 0.0)), 0.0)
    den = p.sum(axis=-1, keepdims=True)
    den = np.where(den > 0, den, 1.0)
    out = np.matmul(p, vv) / den
    absmean = np.matmul(p, np.abs(vv)) / den
    return out.transpose(0, 2, 1, 3).copy(), absmean.transpose(0, 2, 1, 3).copy()


def random_bound(ref, absmean):
    """|out - ref| allowed per element on N(0, 1) data: the probabilities enter the value product rounded to fp16 (relative
    2^-11 each) while the denominator sums the unrounded fp32 values, so the quotient is off by at most 2^-11 sum p |v| /
    sum p; then one rounding to fp16 (half an ulp).  That model with a factor 2."""
    return 2.0 ** -10 * absmean + fp16_ulp(ref)


def bits_differ(out, exp):
    """[...]: any channel whose fp16 bits differ"""
    return (np.ascontiguousarray(out).view(np.int16) != np.ascontiguousarray(exp).view(np.int16)).any(-1)


def _pairs(B, Hkv):
    return np.repeat(np.arange(B), Hkv), np.tile(np.arange(Hkv), B)


def place_keys(k, placed):
    """a copy of k with, for every (rows [B, Hkv], vectors [B, Hkv, D]) of `placed`, row rows[b, h] of head (b, h) replaced"""
    k = k.copy()
    B, Hkv = k.shape[:2]
    ib, ih = _pairs(B, Hkv)
    for rows, vec in placed:
        k[ib, ih, np.asarray(rows).reshape(-1)] = np.asarray(vec).reshape(B * Hkv, -1)
    return k


# ---- staircase -----------------------------------------------------------------------------------------------------------

def staircase_base(B, T, H, Hkv, keys, D, seed):
    """One query vector per (b, kv head), repeated over the T rows and the H / Hkv heads of the group; random keys, values
    without zeros; `hot` beats the random rows by GAP_TARGET, `hotter` beats `hot` by another GAP_TARGET."""
    rng = np.random.default_rng(seed)
    q1 = normal_f16(rng, (B, Hkv, D))
    q = np.ascontiguousarray(np.broadcast_to(expand_heads(q1, H)[:, None], (B, T, H, D)))
    k = poison_tail(normal_f16(rng, (B, Hkv, keys + PREFILL_PAD, D)), keys)
    v = poison_tail(nonzero_normal_f16(rng, (B, Hkv, keys + PREFILL_PAD, D)), keys)
    scale = D ** -0.5
    return dict(q=q, q1=q1, k=k, v=v, keys=keys, scale=scale, hot=hot_keys(q1, scale), hotter=hot_keys(q1, scale, 2 * GAP_TARGET))


def staircase_winner(T, koff, steps):
    """steps: [(rows [B, Hkv], rank)].  [B, Hkv, T]: the row whose value query t must return -- the highest-ranked step among
    those it may attend (row <= t + koff) -- or -1 where every step is still in its future."""
    rows0 = np.asarray(steps[0][0])
    win = np.full(rows0.shape + (T,), -1, dtype=np.int64)
    best = np.full(rows0.shape + (T,), -1, dtype=np.int64)
    lim = np.arange(T) + koff
    for rows, rank in steps:
        take = (np.asarray(rows)[..., None] <= lim) & (rank > best)
        win = np.where(take, np.asarray(rows)[..., None], win)
        best = np.where(take, rank, best)
    return win


def check_staircase(out, case, win, ref, absmean):
    """out [B, T, H, D] against the winners [B, Hkv, T]: bit equality with V[win] where win >= 0, the random bound against the
    reference of the unedited cache (ref, absmean) elsewhere.  Returns (bad [B, T, H] bool, largest bound ratio or 0)."""
    B, T, H, D = out.shape
    Hkv = case["v"].shape[1]
    w = expand_heads(win, H).transpose(0, 2, 1)                                  # [B, T, H]
    vv = expand_heads(case["v"], H)                                               # [B, H, S, D]
    ib, ih = np.arange(B)[:, None, None], np.arange(H)[None, None, :]
    exp = vv[ib, ih, np.maximum(w, 0)]                                            # [B, T, H, D]
    exact = w >= 0
    bad = exact & bits_differ(out, exp)
    err = np.abs(out.astype(np.float64) - ref) / random_bound(ref, absmean)
    err = np.where(exact[..., None], 0.0, err)
    bad |= ~exact & ~(err.max(-1) <= 1.0)                                         # NaN fails
    return bad, float(np.nan_to_num(err, nan=np.inf).max()) if err.size else 0.0


# ---- pairing: diagonal and permutation -------------------------------------------------------------------------------------

def pairing_map(T, keys, koff, kind, rng):
    """pi [T]: 'diagonal' t + koff; 'permutation' uniform over the rows of [0, min(keys - 1, t + koff)] that no earlier query
    took (what redrawing on a collision gives).  With koff = 0 the only injective choice is the diagonal itself."""
    if kind == "diagonal":
        pi = np.arange(T) + koff
        assert pi[0] >= 0 and pi[-1] < keys
        return pi
    used = np.zeros(keys, dtype=bool)
    pi = np.empty(T, dtype=np.int64)
    for t in range(T):
        free = np.flatnonzero(~used[: min(keys, t + koff + 1)])
        pi[t] = free[rng.integers(free.size)]
        used[pi[t]] = True
    return pi


def pairing_gap(q0, k, pi, keys, koff, scale):
    """least margin, over every (b, kv head, t), of query t's own hot score over every OTHER row it may attend (float64)"""
    B, T, Hkv, D = q0.shape
    s = np.matmul(q0.astype(np.float64).transpose(0, 2, 1, 3), k[:, :, :keys].astype(np.float64).transpose(0, 1, 3, 2)) * float(scale)
    own = np.take_along_axis(s, pi[..., None], axis=-1)[..., 0]                   # [B, Hkv, T]
    allowed = np.arange(keys)[None, :] <= (np.arange(T)[:, None] + koff)
    other = np.where(allowed & (np.arange(keys) != pi[..., None]), s, -np.inf).max(-1)
    return float((own - other).min())


def pairing_case(B, T, H, Hkv, keys, koff, D, seed, kind):
    """q N(0, 1) per (b, t, kv head), the same for the heads of a group; key row pi[b, hk, t] = c q[b, t, hk] with the least
    target (a multiple of GAP_TARGET) whose gap over every competitor -- the other queries' hot keys included -- reaches
    GAP_MIN + PAIR_MARGIN.  Needs every query to attend something (t + koff >= 0)."""
    rng = np.random.default_rng(seed)
    q0 = normal_f16(rng, (B, T, Hkv, D))
    base = normal_f16(rng, (B, Hkv, keys + PREFILL_PAD, D))
    v = poison_tail(nonzero_normal_f16(rng, (B, Hkv, keys + PREFILL_PAD, D)), keys)
    pi = np.stack([np.stack([pairing_map(T, keys, koff, kind, rng) for _ in range(Hkv)]) for _ in range(B)])   # [B, Hkv, T]
    scale = D ** -0.5
    ib, ih = np.arange(B)[:, None, None], np.arange(Hkv)[None, :, None]
    for mult in range(1, 9):
        k = base.copy()
        k[ib, ih, pi] = hot_keys(q0, scale, mult * GAP_TARGET).transpose(0, 2, 1, 3)
        gap = pairing_gap(q0, k, pi, keys, koff, scale)
        if gap >= GAP_MIN + PAIR_MARGIN:
            break
    return dict(q=np.repeat(q0, H // Hkv, axis=2), q0=q0, k=poison_tail(k, keys), v=v, pi=pi, keys=keys, scale=scale,
                target=mult * GAP_TARGET, gap=gap)


def check_pairing(out, case):
    """bad [B, T, H]: out[b, t, h] is not V[b, h // groups, pi[b, h // groups, t]] bit for bit"""
    B, T, H, D = out.shape
    w = expand_heads(case["pi"], H).transpose(0, 2, 1)
    vv = expand_heads(case["v"], H)
    exp = vv[np.arange(B)[:, None, None], np.arange(H)[None, None, :], w]
    return bits_differ(out, exp)


# ---- prefix census ---------------------------------------------------------------------------------------------------------

def prefill_census_case(B, T, H, Hkv, keys, D, seed):
    v, k = census_values(B, Hkv, keys + PREFILL_PAD, D, seed)
    return dict(q=np.zeros((B, T, H, D), dtype=np.float16), k=poison_tail(k, keys), v=poison_tail(v, keys), keys=keys,
                scale=D ** -0.5)


def prefix_census_shift_ulps(v, counts):
    """(drop, double): the least census_shift_ulps figure over the prefix lengths in `counts` (lengths 0 show nothing and
    are skipped; length 1 has no `double` figure)."""
    drop, dbl = np.inf, np.inf
    for n in sorted(set(int(c) for c in counts if c > 0)):
        a, b = census_shift_ulps(v, n)
        drop = min(drop, a)
        if b is not None:
            dbl = min(dbl, b)
    return drop, dbl


# ---- random ----------------------------------------------------------------------------------------------------------------
RAMP_RISE = 4.0   # rise of the ramp per 64-key block, in standard deviations of a score


def prefill_random_case(B, T, H, Hkv, keys, D, seed, scale=None, ramp=False, koff=None):
    """N(0, 1) everywhere.  ramp: q += u and k[s] += s g u for one common vector u, g such that the mean score rises by
    RAMP_RISE standard deviations of a score per 64 keys (5.7 natural-log units at scaling D^-0.5, 64 at scaling 1 and
    D = 128: alpha stays above 0 in fp32).  The draw is repeated, with the next stream of the seed, until the block maxima
    of the last query row rise strictly (`block_maxima`; the order of the scores does not depend on the scaling) -- a last
    block of one key exceeds the block before it in about one draw of a hundred."""
    koff = keys - T if koff is None else koff
    for attempt in range(4000):
        rng = np.random.default_rng([seed, attempt])
        q = rng.standard_normal((B, T, H, D), dtype=np.float32)
        k = rng.standard_normal((B, Hkv, keys + PREFILL_PAD, D), dtype=np.float32)
        v = normal_f16(rng, (B, Hkv, keys + PREFILL_PAD, D))
        if ramp:
            u = rng.standard_normal(D, dtype=np.float32)
            g = RAMP_RISE * np.sqrt(2.0 * D) / (64.0 * float((u.astype(np.float64) ** 2).sum()))
            q = q + u
            k = k + (np.arange(keys + PREFILL_PAD, dtype=np.float32) * np.float32(g))[:, None] * u
        q, k = q.astype(np.float16), k.astype(np.float16)
        if not ramp or prefill_counts(T, keys, koff)[-1] == 0 or (np.diff(block_maxima(q, k, keys, koff, 1.0), axis=-1) > 0).all():
            break
    else:
        raise AssertionError("no ramp with rising block maxima found")
    return dict(q=q, k=poison_tail(k, keys), v=poison_tail(v, keys), keys=keys, scale=D ** -0.5 if scale is None else float(scale))


def block_maxima(q, k, keys, koff, scale, block=64):
    """float64 maxima of the LAST query row's scores over each block of `block` keys it attends: [B, H, blocks]"""
    B, T, H, D = q.shape
    n = int(prefill_counts(T, keys, koff)[-1])
    kk = expand_heads(np.asarray(k)[:, :, :n], H).astype(np.float64)
    s = np.einsum("bhd,bhsd->bhs", np.asarray(q)[:, -1].astype(np.float64), kk) * float(scale)
    return np.stack([s[..., i: i + block].max(-1) for i in range(0, n, block)], axis=-1)
