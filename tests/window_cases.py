"""Inputs, references and checks for SLIDING-WINDOW attention: a query at cache row p attends rows
max(0, p - W + 1) .. p.  A plain module for the tests (not a conftest), NumPy only, CPU only; it builds on attn_cases.py and shares
no code with the kernels.  Pinned on the CPU by test_window_cases_cpu.py.

  window_reference   attn_cases.prefill_reference with the lower bound.
  window_counts      rows every query attends.
  staircase          hot keys whose rank FALLS with the row index (the oldest placed row is the hottest): a query must return V of
                     the oldest placed row inside its window, bit for bit -- a key leaked from just below the window is older,
                     hence hotter, and wins.
  census             q = 0: the mean of the small-integer V rows of the window.
"""
import numpy as np

import attn_cases as ac

# ---- the shapes the GPU tests use (test_gpu_window_attn.py) ------------------------------------------------------------------
B, H, HKV = 2, 4, 2
DIMS = (64, 128)
# (name, query rows, keys): a fresh prompt of two query blocks, the second ragged; 40 rows behind 260 cached ones
SHAPES = {"fresh": (160, 160), "behind": (40, 300)}


def windows(keys):
    return (1, 5, 64, 65, 129, keys, keys + 7)


# Placed rows, oldest first (rank falls with the row index).  Every pair (r, r + 1) is a window edge for the query at cache row
# p = r + W: r sits at p - W (outside), r + 1 at p - W + 1 (inside).  Pairs straddle the 64-key block boundaries (63 | 64, 191 | 192,
# 255 | 256), and the queries they are an edge for straddle the waves' 32-row boundaries (fresh: 31 + W, 63 + W, 95 + W for W = 64, 65,
# and 0 + 129 = t 129 | 128; behind 260 rows: t = 31 | 32 is p = 291 | 292, edges 286 | 287 and 287 | 288 for W = 5).
PLACED = {"fresh": (0, 1, 30, 31, 32, 63, 64, 95, 96), "behind": (133, 134, 191, 192, 199, 200, 255, 256, 270, 271, 286, 287, 288)}


def window_counts(T, keys, koff, W):
    """rows every query attends: those of [max(0, p - W + 1), min(keys, p + 1)), p = t + koff; at least 0"""
    p = np.arange(T) + koff
    return np.maximum(np.minimum(keys, p + 1) - np.maximum(0, p - W + 1), 0)


def window_allowed(T, keys, koff, W):
    """[T, keys] bool: may query t attend row s"""
    s, p = np.arange(keys)[None, :], (np.arange(T) + koff)[:, None]
    return (s <= p) & (s > p - W)


def window_reference(q, k, v, keys, koff, W, scale):
    """attn_cases.prefill_reference over the rows s < keys, s <= t + koff and s > t + koff - W.  Returns (out, absmean)."""
    Bq, T, Hq, D = q.shape
    kk = ac.expand_heads(np.asarray(k)[:, :, :keys], Hq).astype(np.float64)
    vv = ac.expand_heads(np.asarray(v)[:, :, :keys], Hq).astype(np.float64)
    s = np.matmul(np.asarray(q).astype(np.float64).transpose(0, 2, 1, 3), kk.transpose(0, 1, 3, 2)) * float(scale)
    allowed = window_allowed(T, keys, koff, W)
    s = np.where(allowed, s, -np.inf)
    vv = np.where(np.isfinite(vv), vv, 0.0)     # rows no query may attend can hold anything (0 * NaN)
    top = s.max(axis=-1, keepdims=True)
    alive = np.isfinite(top)
    with np.errstate(invalid="ignore"):
        p = np.where(alive & allowed, np.exp(s - np.where(alive, top, 0.0)), 0.0)
    den = p.sum(axis=-1, keepdims=True)
    den = np.where(den > 0, den, 1.0)
    out = np.matmul(p, vv) / den
    absmean = np.matmul(p, np.abs(vv)) / den
    return out.transpose(0, 2, 1, 3).copy(), absmean.transpose(0, 2, 1, 3).copy()


# ---- oldest-wins staircase -------------------------------------------------------------------------------------------------

def staircase_case(shape, D, seed):
    """attn_cases.staircase_base with the rows PLACED[shape] made hot, the oldest the hottest: row i of n gets the hot key of
    strength (n - i) * GAP_TARGET.  Returns the case with `placed` (rows) and `ranks`."""
    T, keys = SHAPES[shape]
    c = ac.staircase_base(B, T, H, HKV, keys, D, seed)
    rows = PLACED[shape]
    n = len(rows)
    k = c["k"].copy()
    for i, r in enumerate(rows):
        k[:, :, r] = ac.hot_keys(c["q1"], c["scale"], (n - i) * ac.GAP_TARGET)
    c.update(k=k, placed=np.asarray(rows), ranks=np.arange(n, 0, -1), T=T, koff=keys - T)
    return c


def staircase_gap(case):
    """least float64 margin between the scores of consecutive ranks, and of the lowest rank over every ordinary row"""
    keys, rows = case["keys"], case["placed"]
    s = ac.scores(ac.expand_heads(case["q1"], H), case["k"][:, :, :keys], case["scale"])      # [B, H, keys]
    placed = s[..., rows]                                                                     # falling with the index
    other = np.delete(s, rows, axis=-1).max(-1)
    return float(min((placed[..., :-1] - placed[..., 1:]).min(), (placed[..., -1] - other).min()))


def window_winner(T, koff, W, rows, ranks):
    """[T]: the highest-ranked placed row inside (p - W, p], p = t + koff, or -1 where the window holds none"""
    p = np.arange(T) + koff
    win = np.full(T, -1, dtype=np.int64)
    best = np.full(T, -1, dtype=np.int64)
    for r, rank in zip(rows, ranks):
        take = (r <= p) & (r > p - W) & (rank > best)
        win = np.where(take, r, win)
        best = np.where(take, rank, best)
    return win


def edge_queries(T, koff, W, rows):
    """queries t for which some placed row sits at p - W (just outside) while p - W + 1 (just inside) is placed too"""
    have = set(int(r) for r in rows)
    p = np.arange(T) + koff
    return np.array([t for t in range(T) if (p[t] - W) in have and (p[t] - W + 1) in have], dtype=np.int64)


def check_window_staircase(out, case, W, ref, absmean):
    """out [B, T, H, D]: bit equality with V[winner] where the window holds a placed row, the random bound against the windowed
    reference (ref, absmean: of the edited cache) elsewhere.  Returns bad [B, T, H]."""
    win = window_winner(case["T"], case["koff"], W, case["placed"], case["ranks"])
    w = np.broadcast_to(win[None, None, :], (B, HKV, case["T"]))
    bad, _ = ac.check_staircase(out, case, w, ref, absmean)
    return bad, win


# ---- window census -----------------------------------------------------------------------------------------------------------

def census_case(shape, D, seed):
    T, keys = SHAPES[shape]
    c = ac.prefill_census_case(B, T, H, HKV, keys, D, seed)
    c.update(T=T, koff=keys - T)
    return c


def window_census_mean(v, T, keys, koff, W):
    """float64 [B, T, Hkv, D]: the mean of the window's V rows (zeros where the window is empty)"""
    x = np.asarray(v)[:, :, :keys].astype(np.float64)
    cs = np.concatenate([np.zeros_like(x[:, :, :1]), np.cumsum(x, axis=2)], axis=2)
    p = np.arange(T) + koff
    lo, hi = np.maximum(0, p - W + 1), np.minimum(keys, p + 1)
    n = np.maximum(hi - lo, 0)
    tot = cs[:, :, np.maximum(hi, lo)] - cs[:, :, lo]                               # [B, Hkv, T, D]
    return (tot / np.maximum(n, 1)[None, None, :, None]).transpose(0, 2, 1, 3)


def window_census_shift_ulps(v, T, keys, koff, W):
    """attn_cases.census_shift_ulps over every query's window: (drop, double), the least figures over the queries (None where
    every window holds one row: no `double` figure)."""
    x = np.asarray(v)[:, :, :keys].astype(np.float64)
    p = np.arange(T) + koff
    drop, dbl = np.inf, np.inf
    for t in range(T):
        lo, hi = max(0, p[t] - W + 1), min(keys, p[t] + 1)
        if hi <= lo:
            continue
        a, b = ac.census_shift_ulps(x[:, :, lo:hi], hi - lo)
        drop = min(drop, a)
        if b is not None:
            dbl = min(dbl, b)
    return drop, (None if dbl == np.inf else dbl)


# ---- decode: the last W of n rows ----------------------------------------------------------------------------------------------

def decode_window_start(n, W, start=0):
    """the first row a decode step with n valid rows (the new token included) attends: max(start, n - W), at least 0"""
    return max(int(start), n - W, 0)
