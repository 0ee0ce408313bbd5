"""Prompt attention (eetq_amd/csrc/attn_prefill.hip) at the shapes where its paths change, with inputs on which ONE lost,
doubled or misplaced key, an off-by-one at the causal diagonal or a wrong `edge` decision shows: the four prompt families
of tests/attn_cases.py against its float64 reference, at D = 128 and D = 64.

  staircase    identical queries, key row r hot: out[t] == V[r] BIT FOR BIT for every t with t + koff >= r, r swept over
               every row (a different r in every (batch, kv head) of a launch); earlier rows within the random bound
  pairing      distinct queries, key row pi(t) hot for query t (the diagonal t + koff, and a random injective map):
               out[t] == V[pi(t)] BIT FOR BIT for all t of one launch
  census       q = 0: out[t] within 1 fp16 ulp of the float64 mean of V[0 .. min(keys, t + koff + 1) - 1]
  random       |out - ref| <= 2^-10 sum p |v| / sum p + fp16_ulp(ref) per element (attn_cases.random_bound), scaling D^-0.5
               and 1.0, plain and with a ramp that moves the running maximum in every block

Every cache is PREFILL_PAD rows longer than `keys` and NaN there; no output may be NaN.  The family drivers below take the
attention as a function of NumPy arrays, so that tests/test_attn_prefill_cases_cpu.py runs the very same checks on a NumPy
emulation of the kernel's arithmetic and on its mutants.  The coverage guard restates the kernel's launch arithmetic (nqb,
kend, nblk, the per-wave `active` and `edge`) and fails when a table row no longer reaches what it claims; it is never a
source of expected values.

233 cases (the guard among them), 4.2 s wall for the file on an MI355X.  Largest figures per table row, D = 128 / D = 64:

  row   random: |out - ref| / bound   census: error in fp16 ulp   staircase bait rows: |out - ref| / bound
  1     0.461 / 0.458                 0.4984 / 0.4984             0.429 / 0.389
  2     0.430 / 0.433                 0.4979 / 0.4979             0.228 / 0.241
  3     0.448 / 0.455                 0.4961 / 0.4960             0.386 / 0.407
  4     0.222 / 0.263                 0.4857 / 0.4857             --
  5     0.447 / 0.387                 0.4963 / 0.4962             --
  6     0.462 / 0.444                 0.4933 / 0.4933             (no bait rows)
  7     0.430 / 0.433                 0.4979 / 0.4979             0.228 / 0.241   (the same in all three layouts)

Paths first executed under test here: K and V with a row stride other than D ([B, S, Hkv, D] storage and a D + 8 pitch, so the
buffer descriptor's length with k_ss != D), explicit `scaling` other than the default, explicit `causal_offset` (negative, and
beyond keys - T), a workgroup with nblk == 0, queries with nothing to attend, launches without any causal cut (every block but
the last interior), keys = T at 63, 65, 127 and 129.

Found and fixed: the kernel handed its probabilities to the second product as plain fp16 p <= 1; below 2^-14 those are fp16
subnormals with an absolute error of up to 2^-25 each, which the random bound (relative 2^-11) does not cover.  Rows 2 and 7 at
D = 64, scaling 1 with the ramp measured 1.214 of the bound on one element (b 1, t 112, h 3, channel 49: an answer of 1.7e-5
off by 1.03e-7), and 0.719 at D = 128, scaling 1; every bit-for-bit and census assertion passed as the kernel stood.  The
kernel now carries 2^12 p (attn_prefill.hip, kPfPShift), which took those two figures to 0.433 and 0.430;
tests/test_attn_prefill_cases_cpu.py::test_unshifted_probabilities_miss_the_random_bound keeps the old arithmetic as a mutant.
"""
import collections
import functools

import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (128, 64)

Shape = collections.namedtuple("Shape", "B T H Hkv keys koff")   # koff None: the wrapper's default, keys - T


def koff_of(s):
    return s.keys - s.T if s.koff is None else s.koff


ROWS = {
    1: [Shape(2, 320, 8, 8, 320, None)],                                   # 3 query blocks (last half full), 5 key blocks
    2: [Shape(2, 200, 8, 4, 237, None)],                                   # append behind 37 rows, grouped heads, ragged
    3: [Shape(1, n, 2, 1, n, None) for n in (63, 64, 65, 127, 128, 129)],  # either side of a key / query block edge
    4: [Shape(1, 1, 2, 2, 70, None)],                                      # one query row
    5: [Shape(1, 140, 2, 2, 140, -5), Shape(1, 140, 2, 2, 140, -140)],     # rows (and a workgroup) with nothing to attend
    6: [Shape(1, 100, 4, 2, 150, 1000)],                                   # no causal cut: interior blocks, key < Tk only
    7: [Shape(2, 200, 8, 4, 237, None)],                                   # row 2 through strided K / V / q (LAYOUTS)
}
LAYOUTS = ("bshd", "pitch", "fusedq")


# ---- the kernel's launch arithmetic, restated (guard only) -----------------------------------------------------------------
BM, BN, WAVE_ROWS = 128, 64, 32


def geometry(s):
    """[(query block, nblk, [(j, [(wave, active, edge) of the waves that own a real query row])])]"""
    koff, out = koff_of(s), []
    nqb = -(-s.T // BM)
    for qb in range(nqb):
        q0 = qb * BM
        kend = min(s.keys, q0 + BM + koff)
        nblk = -(-kend // BN) if kend > 0 else 0
        blocks = []
        for j in range(nblk):
            key0 = j * BN
            waves = [(w, key0 <= q0 + w * WAVE_ROWS + WAVE_ROWS - 1 + koff,
                      key0 + BN - 1 > q0 + w * WAVE_ROWS + koff or key0 + BN > s.keys)
                     for w in range(BM // WAVE_ROWS) if q0 + w * WAVE_ROWS < s.T]
            blocks.append((j, waves))
        out.append((qb, nblk, blocks))
    return out


def reach(s):
    g = geometry(s)
    return dict(
        nqb=len(g), nblk=[n for _, n, _ in g],
        skip=any(any(not a for _, a, _ in w) and any(a for _, a, _ in w) for _, _, bl in g for _, w in bl),
        interior=any(a and not e for _, _, bl in g for _, w in bl for _, a, e in w),
        edge=any(a and e for _, _, bl in g for _, w in bl for _, a, e in w))


def check_coverage():
    """Every row of the table reaches what its comment claims."""
    (s,) = ROWS[1]
    r = reach(s)
    assert r["nqb"] == 3 and s.T % BM == BM // 2 and max(r["nblk"]) >= 5 and r["skip"] and r["interior"] and s.H * s.B == 16
    assert koff_of(s) == 0
    (s,) = ROWS[2]
    r = reach(s)
    assert koff_of(s) == 37 and all(37 % m for m in (4, 32, 64)) and s.H // s.Hkv == 2 and s.T % 32 and s.keys % 64
    assert r["nqb"] == 2 and r["skip"] and r["interior"]
    assert sorted(x.keys for x in ROWS[3]) == [63, 64, 65, 127, 128, 129] and all(x.T == x.keys and x.koff is None for x in ROWS[3])
    assert [reach(x)["nqb"] for x in ROWS[3]] == [1, 1, 1, 1, 1, 2] and [max(reach(x)["nblk"]) for x in ROWS[3]] == [1, 1, 2, 2, 2, 3]
    (s,) = ROWS[4]
    assert s.T == 1 and koff_of(s) == s.keys - 1 and reach(s)["nblk"] == [2]
    a, b = ROWS[5]
    assert 0 in reach(b)["nblk"] and any(n > 0 for n in reach(b)["nblk"]), "a whole workgroup with nblk == 0, another with work"
    assert (ac.prefill_counts(a.T, a.keys, a.koff) == 0).sum() == 5 and (ac.prefill_counts(b.T, b.keys, b.koff) == 0).all()
    (s,) = ROWS[6]
    r = reach(s)
    assert r["nblk"] == [3] and r["interior"] and r["edge"] and not r["skip"] and s.koff > s.keys
    assert all(all(not e for _, _, e in w) for _, _, bl in geometry(s) for j, w in bl if j < 2), "only the last block is an edge"
    assert ROWS[7] == ROWS[2]
    every = [x for cases in ROWS.values() for x in cases]
    assert any(0 in reach(x)["nblk"] for x in every) and any(max(reach(x)["nblk"]) >= 5 for x in every)
    assert all(x.keys <= 320 and x.T <= 320 for x in every)


def test_coverage_guard():
    check_coverage()


# ---- cases: built once per (shape, D) on the host ----------------------------------------------------------------------------

def _seed(s, D, salt):
    return 100003 * salt + 1009 * s.T + 31 * s.keys + 7 * s.B + D + (0 if s.koff is None else 13 * (s.koff % 997))


@functools.lru_cache(maxsize=None)
def staircase_case(s, D):
    c = ac.staircase_base(s.B, s.T, s.H, s.Hkv, s.keys, D, _seed(s, D, 1))
    c["ref"], c["absmean"] = ac.prefill_reference(c["q"], c["k"], c["v"], s.keys, koff_of(s), c["scale"])
    return c


@functools.lru_cache(maxsize=None)
def pairing_case(s, D, kind):
    return ac.pairing_case(s.B, s.T, s.H, s.Hkv, s.keys, koff_of(s), D, _seed(s, D, 2 if kind == "diagonal" else 3), kind)


@functools.lru_cache(maxsize=None)
def census_case(s, D):
    c = ac.prefill_census_case(s.B, s.T, s.H, s.Hkv, s.keys, D, _seed(s, D, 4))
    c["ref"], _ = ac.prefill_reference(c["q"], c["k"], c["v"], s.keys, koff_of(s), c["scale"])
    return c


RANDOM_KINDS = (("default", False), ("default", True), ("one", False), ("one", True))   # (scaling, ramp)


@functools.lru_cache(maxsize=None)
def random_case(s, D, scaling, ramp):
    c = ac.prefill_random_case(s.B, s.T, s.H, s.Hkv, s.keys, D, _seed(s, D, 5 + ramp), scale=None if scaling == "default" else 1.0,
                               ramp=ramp, koff=koff_of(s))
    c["explicit_scale"] = None if scaling == "default" else 1.0
    c["ref"], c["absmean"] = ac.prefill_reference(c["q"], c["k"], c["v"], s.keys, koff_of(s), c["scale"])
    return c


# ---- family drivers: `attend(q, k, v, keys, koff, scale)` -> float16 [B, T, H, D]; koff / scale None = the default ------------

def _first(bad, what):
    idx = np.argwhere(bad)
    return "%d of %d %s wrong; first (b, t, h): %s" % (bad.sum(), bad.size, what, ", ".join(str(tuple(int(i) for i in x)) for x in idx[:6]))


def _steps_launch(attend, s, c, steps):
    """steps: [(rows [B, Hkv], vectors [B, Hkv, D], rank)] placed in the cache for one launch"""
    k = ac.place_keys(c["k"], [(r, vec) for r, vec, _ in steps])
    out = attend(c["q"], k, c["v"], s.keys, s.koff, None)
    assert not np.isnan(out).any(), "NaN in the output"
    win = ac.staircase_winner(s.T, koff_of(s), [(r, rank) for r, _, rank in steps])
    bad, ratio = ac.check_staircase(out, c, win, c["ref"], c["absmean"])
    return bad, ratio


def drive_staircase_sweep(attend, s, D):
    """The hot key at every row of [0, keys) in turn, a different row in every (batch, kv head) of a launch."""
    c = staircase_case(s, D)
    heads, worst = s.B * s.Hkv, 0.0
    for launch in range(ac.sweep_launches(s.keys, heads)):
        r = ac.sweep(s.keys, heads, launch).reshape(s.B, s.Hkv)
        bad, ratio = _steps_launch(attend, s, c, [(r, c["hot"], 1)])
        worst = max(worst, ratio)
        assert not bad.any(), "hot rows %s: %s" % (r.reshape(-1).tolist(), _first(bad, "query rows"))
    return worst


def edge_rows(keys):
    """row 0, the rows around every 32- and 64-key edge, the last row"""
    rows = [0, keys - 1]
    for e in range(32, keys + 1, 32):
        rows += [e - 1, e, e + 1]
    return sorted(set(x for x in rows if 0 <= x < keys))


def step_pairs(keys):
    """(r1, r2), r1 < r2: neighbours inside a block, across a block edge, a block apart, the two ends"""
    pairs = [(0, keys - 1), (keys // 2, keys // 2 + 1), (62, 65), (63, 64), (5, 5 + 64), (keys - 2, keys - 1), (0, 1), (63, 128)]
    return [(a, b) for a, b in pairs if 0 <= a < b < keys]


def drive_staircase_edges(attend, s, D):
    """A few hot rows straddling each block edge, then the two-step variants: hot at r1 and hotter at r2 > r1 (rows between
    the steps return V[r1], later ones V[r2]: alpha is exactly 0 across blocks), hotter at r1 and hot at r2 (every row from r1
    on returns V[r1]: a later, weaker block adds exactly nothing)."""
    c = staircase_case(s, D)
    heads, worst = s.B * s.Hkv, 0.0
    rows = edge_rows(s.keys)
    for i in range(0, len(rows), heads):
        r = np.resize(np.array(rows[i: i + heads]), heads).reshape(s.B, s.Hkv)
        bad, ratio = _steps_launch(attend, s, c, [(r, c["hot"], 1)])
        worst = max(worst, ratio)
        assert not bad.any(), "hot rows %s: %s" % (r.reshape(-1).tolist(), _first(bad, "query rows"))
    pairs = step_pairs(s.keys)
    for i in range(0, len(pairs), heads):
        pr = np.resize(np.array(pairs[i: i + heads]), (heads, 2))
        r1, r2 = pr[:, 0].reshape(s.B, s.Hkv), pr[:, 1].reshape(s.B, s.Hkv)
        for first, second, name in ((("hot", 1), ("hotter", 2), "hot then hotter"), (("hotter", 2), ("hot", 1), "hotter then hot")):
            bad, ratio = _steps_launch(attend, s, c, [(r1, c[first[0]], first[1]), (r2, c[second[0]], second[1])])
            worst = max(worst, ratio)
            assert not bad.any(), "%s at %s: %s" % (name, pr.tolist(), _first(bad, "query rows"))
    return worst


def drive_pairing(attend, s, D, kind):
    c = pairing_case(s, D, kind)
    out = attend(c["q"], c["k"], c["v"], s.keys, s.koff, None)
    assert not np.isnan(out).any(), "NaN in the output"
    bad = ac.check_pairing(out, c)
    assert not bad.any(), "%s: %s" % (kind, _first(bad, "query rows do not return V[pi(t)] bit for bit and are"))


def drive_census(attend, s, D):
    """Within ONE fp16 ulp of the float64 mean: l = the count and sum V are exact in fp32, so the only roundings are the fp32
    reciprocal, the fp32 product with it (together under 2^-23 relative, a 2^-12 part of an fp16 ulp) and the rounding to
    fp16 (half an ulp).  Rows with nothing to attend give zeros."""
    c = census_case(s, D)
    out = attend(c["q"], c["k"], c["v"], s.keys, s.koff, None)
    assert not np.isnan(out).any(), "NaN in the output"
    err = np.abs(out.astype(np.float64) - c["ref"]) / ac.fp16_ulp(c["ref"])
    empty = ac.prefill_counts(s.T, s.keys, koff_of(s)) == 0
    assert not out[:, empty].any(), "a query with nothing to attend must give zeros"
    bad = ~(err.max(-1) <= 1.0)
    assert not bad.any(), "max error %.3f ulp; %s" % (err.max(), _first(bad, "query rows"))
    return float(err.max())


def drive_random(attend, s, D, scaling, ramp):
    c = random_case(s, D, scaling, ramp)
    out = attend(c["q"], c["k"], c["v"], s.keys, s.koff, c["explicit_scale"])
    assert not np.isnan(out).any(), "NaN in the output"
    ratio = np.abs(out.astype(np.float64) - c["ref"]) / ac.random_bound(c["ref"], c["absmean"])
    empty = ac.prefill_counts(s.T, s.keys, koff_of(s)) == 0
    assert not out[:, empty].any(), "a query with nothing to attend must give zeros"
    bad = ~(ratio.max(-1) <= 1.0)
    assert not bad.any(), "max |out - ref| / bound %.3f; %s" % (ratio.max(), _first(bad, "query rows"))
    return float(ratio.max())


# ---- the GPU side ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.prefill_attention is None:
        pytest.skip("prefill_attention lives in the compiled module")
    return o


def _lay_q(q, layout):
    """fusedq: the query as the strided view of a fused QKV row (other columns NaN)"""
    t = torch.from_numpy(q).to(DEV)
    if layout != "fusedq":
        return t
    B, T, H, D = q.shape
    fused = torch.full((B, T, (H + 4) * D), float("nan"), dtype=torch.float16, device=DEV)
    view = fused[..., : H * D].unflatten(-1, (H, D))
    view.copy_(t)
    assert not view.is_contiguous() and view.stride(1) == (H + 4) * D
    return view


def _lay_kv(x, layout):
    """bshd: [B, S, Hkv, D] storage viewed [B, Hkv, S, D]; pitch: rows D + 8 apart (the gap NaN)"""
    t = torch.from_numpy(x).to(DEV)
    B, Hkv, S, D = x.shape
    if layout == "bshd":
        view = torch.empty((B, S, Hkv, D), dtype=torch.float16, device=DEV).permute(0, 2, 1, 3)
        assert view.stride(2) == Hkv * D and view.stride(1) == D
    elif layout == "pitch":
        view = torch.full((B, Hkv, S, D + 8), float("nan"), dtype=torch.float16, device=DEV)[..., :D]
        assert view.stride(2) == D + 8
    else:
        return t
    view.copy_(t)
    assert not view.is_contiguous()
    return view


def gpu_attend(ops, layout="plain"):
    def attend(q, k, v, keys, koff, scale):
        kw = {}
        if koff is not None:
            kw["causal_offset"] = koff
        if scale is not None:
            kw["scaling"] = scale
        out = ops.prefill_attention(_lay_q(q, layout), _lay_kv(k, layout), _lay_kv(v, layout), keys, **kw)
        assert out.shape == q.shape and out.is_contiguous()
        return out.cpu().numpy()
    return attend


def _cases(rows, layouts=("plain",)):
    return [(r, i, D, lay) for r in rows for i in range(len(ROWS[r])) for D in DIMS for lay in (LAYOUTS if r == 7 else layouts)]


def _ids(cases):
    out = []
    for r, i, D, lay in cases:
        s = ROWS[r][i]
        out.append("row%d-T%d-keys%d-koff%s-D%d%s" % (r, s.T, s.keys, "dflt" if s.koff is None else s.koff, D,
                                                       "" if lay == "plain" else "-" + lay))
    return out


SWEEP = _cases((1, 2))
EDGES = _cases((3, 6, 7))
DIAGONAL = _cases((1, 2, 3, 4, 7))          # pi(t) = t + koff needs 0 <= t + koff < keys for every t
PERMUTATION = _cases((1, 2, 3, 4, 6, 7))    # needs t + koff >= 0 for every t
EVERY = _cases((1, 2, 3, 4, 5, 6, 7))


@pytest.mark.parametrize("row,i,D,layout", SWEEP, ids=_ids(SWEEP))
def test_staircase_every_row(ops, row, i, D, layout):
    worst = drive_staircase_sweep(gpu_attend(ops, layout), ROWS[row][i], D)
    print("prefill-edges staircase-bait row %d D=%d: max ratio %.3f" % (row, D, worst))


@pytest.mark.parametrize("row,i,D,layout", EDGES, ids=_ids(EDGES))
def test_staircase_block_edges_and_two_steps(ops, row, i, D, layout):
    worst = drive_staircase_edges(gpu_attend(ops, layout), ROWS[row][i], D)
    print("prefill-edges staircase-bait row %d D=%d %s: max ratio %.3f" % (row, D, layout, worst))


@pytest.mark.parametrize("row,i,D,layout", DIAGONAL, ids=_ids(DIAGONAL))
def test_diagonal(ops, row, i, D, layout):
    drive_pairing(gpu_attend(ops, layout), ROWS[row][i], D, "diagonal")


@pytest.mark.parametrize("row,i,D,layout", PERMUTATION, ids=_ids(PERMUTATION))
def test_permutation(ops, row, i, D, layout):
    drive_pairing(gpu_attend(ops, layout), ROWS[row][i], D, "permutation")


@pytest.mark.parametrize("row,i,D,layout", EVERY, ids=_ids(EVERY))
def test_prefix_census(ops, row, i, D, layout):
    s = ROWS[row][i]
    worst = drive_census(gpu_attend(ops, layout), s, D)
    print("prefill-edges census row %d T=%d koff=%s D=%d %s: max error %.4f ulp" % (row, s.T, s.koff, D, layout, worst))


@pytest.mark.parametrize("scaling,ramp", RANDOM_KINDS, ids=["%s%s" % (a, "-ramp" if b else "") for a, b in RANDOM_KINDS])
@pytest.mark.parametrize("row,i,D,layout", EVERY, ids=_ids(EVERY))
def test_random(ops, row, i, D, layout, scaling, ramp):
    s = ROWS[row][i]
    worst = drive_random(gpu_attend(ops, layout), s, D, scaling, ramp)
    print("prefill-edges random row %d T=%d koff=%s D=%d %s scaling=%s ramp=%d: max ratio %.4f" % (row, s.T, s.koff, D, layout, scaling,
                                                                                                  ramp, worst))


@pytest.mark.parametrize("row,i,D,layout", _cases((1, 2, 5)), ids=_ids(_cases((1, 2, 5))))
def test_repeatable_and_default_scaling(ops, row, i, D, layout):
    """A second call returns the same bits, and so does scaling = D^-0.5 (and causal_offset = keys - T) given explicitly."""
    s = ROWS[row][i]
    c = random_case(s, D, "default", True)
    attend = gpu_attend(ops, layout)
    first = attend(c["q"], c["k"], c["v"], s.keys, s.koff, None)
    again = attend(c["q"], c["k"], c["v"], s.keys, s.koff, None)
    explicit = attend(c["q"], c["k"], c["v"], s.keys, koff_of(s), D ** -0.5)
    assert np.array_equal(first.view(np.int16), again.view(np.int16))
    assert np.array_equal(first.view(np.int16), explicit.view(np.int16))
