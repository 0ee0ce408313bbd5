"""Prompt attention behind int8 cache rows (eetq_prefill_attention_i8kv_f16: the KV8 instantiations of eetq_amd/csrc/attn_prefill.hip)
at D = 128 and D = 64, at the shapes of tests/test_gpu_attn_prefill_edges.py (ROWS, keys <= 320) and of
tests/test_gpu_attn_prefill_append.py (SPLIT, keys <= 340).  The inputs are the four prompt families of tests/attn_cases.py turned
into int8 bytes and fp16 scales by the NumPy quantiser of tests/kv8_cases.py; the references are attn_cases.prefill_reference in
float64 on kv8_cases.dequantize_rows, and kv8_cases.hot_value.  They share no code with the kernel.

  staircase    the QUANTISED hot key (bytes and K scale travel together) at the edge rows and two-step pairs of `edges`:
               out[t] == fp16(vs[r] * v8[r]) BIT FOR BIT for every t that sees row r; the >= GAP_MIN gaps are asserted on the
               dequantised rows; bait rows within the random bound
  by K scale   rows r - 1 and r + 1 carry the hot row's bytes with an eighth of its K scale (exact): the row wins by its scale
               alone, a key paired with a neighbour's scale returns a neighbour's V row
  pairing      diagonal and permutation, each bit for bit
  census       q = 0, integer V bytes, V scales cycling 0.5 / 1 / 2 by row: within 1 fp16 ulp of the float64 mean; rows with
               nothing to attend give zeros
  random       |out - ref| <= attn_cases.random_bound(ref, absmean) + 2^-11 absmean + 2^-25: the existing bound covers the
               probabilities' rounding, the added term is the worst case of the ONE fp16 rounding of every vs * v8 (relative
               2^-11 in the normal range, absolute 2^-25 below it)
  device length, split (NaN- and zero-filled workspace, splits=None), three chunks against one cache, layouts, refusals

Every cache is PREFILL_PAD rows longer than `keys`; those rows hold bytes 0x80 and NaN scales.  No output may be NaN.  The int8
entry has no causal_offset argument (the offset is keys - query rows): a table row with an explicit offset runs through
kv_len = T + koff as in the split tests of the fp16 file, and row 6 of `edges` (an offset beyond the cache) has no form here.
The family drivers take the attention as a function of NumPy arrays; tests/test_attn_prefill_i8kv_cpu.py runs them on a NumPy
emulation of the new arithmetic and on its mutants.

325 cases, 5.7 s wall for the file on an MI355X.  Largest figures per table row, D = 128 / D = 64 (random: |out - ref| / bound over
the four kinds; census: fp16 ulp; bait: staircase rows before the hot key, |out - ref| / bound):

  row / split case              random          census            bait
  1                             0.474 / 0.511   0.4984 / 0.4984   0.434 / 0.353
  2 and 7 (both layouts)        0.514 / 0.476   0.4979 / 0.4979   0.222 / 0.234
  3                             0.461 / 0.467   0.4961 / 0.4961   0.359 / 0.357
  4                             0.321 / 0.314   0.4857 / 0.4857   --
  5                             0.550 / 0.427   0.4963 / 0.4963   0.354 / 0.296
  T40-keys340 splits 2, 3, 4    0.398 / 0.447   0.4985 / 0.4985   0.112 / 0.109
  T40-keys130 splits 8          0.475 / 0.409   0.4961 / 0.4961   0.161 / 0.175
  T1-keys70 splits 2            0.321 / 0.314   0.4857 / 0.4857   (no bait rows)
  T129-keys329 splits 2         0.435 / 0.422   0.4984 / 0.4985   0.090 / 0.107
  T129-keys321 splits 2         0.408 / 0.423   0.4984 / 0.4984   0.122 / 0.109
  T140-keys140-koff-5 splits 2  0.550 / 0.427   0.4963 / 0.4963   0.354 / 0.296

Every bit-for-bit family (staircase, by K scale, diagonal, permutation, device length, chunks, workspace fill, the rule) passed as
the kernel was first written.
"""
import functools

import numpy as np
import pytest
import torch

import attn_cases as ac
import kv8_cases as k8c
import test_gpu_attn_prefill_append as app
import test_gpu_attn_prefill_edges as edges
from test_gpu_attn_prefill_edges import koff_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = edges.DIMS
PAD = ac.PREFILL_PAD
TABLE_ROWS = (1, 2, 3, 4, 5, 7)       # row 6: causal_offset = 1000 beyond the cache, which kv_len cannot express


def bound8(ref, absmean):
    """attn_cases.random_bound plus the one fp16 rounding of every vs * v8: relative 2^-11 of sum p |v| / sum p in the normal
    range, absolute 2^-25 (half the subnormal spacing) below it"""
    return ac.random_bound(ref, absmean) + 2.0 ** -11 * absmean + 2.0 ** -25


# ---- int8 caches of the fp16 families -------------------------------------------------------------------------------------------

def pad_rows(x8, s, keys):
    """bytes [B, Hkv, keys, D] and scales [B, Hkv, keys] -> PAD further rows of bytes 0x80 and NaN scales"""
    B, Hkv, _, D = x8.shape
    return (np.concatenate([x8, np.full((B, Hkv, PAD, D), -128, dtype=np.int8)], axis=2),
            np.concatenate([s, np.full((B, Hkv, PAD), np.nan, dtype=np.float16)], axis=2))


def quantize_case(k, v, keys):
    """fp16 caches [B, Hkv, >= keys, D] -> dict(k8, v8 [B, Hkv, keys + PAD, D], sc [B, Hkv, keys + PAD, 2], kd, vd float64
    [B, Hkv, keys, D], hv = fp16(vs * v8) [B, Hkv, keys, D])"""
    k8, ks = k8c.quantize_rows(k[:, :, :keys])
    v8, vs = k8c.quantize_rows(v[:, :, :keys])
    return from_bytes(k8, ks, v8, vs, keys)


def from_bytes(k8, ks, v8, vs, keys):
    kd, vd, hv = k8c.dequantize_rows(k8, ks), k8c.dequantize_rows(v8, vs), k8c.hot_value(v8, vs)
    k8p, ksp = pad_rows(k8, ks, keys)
    v8p, vsp = pad_rows(v8, vs, keys)
    return dict(k8=k8p, v8=v8p, sc=k8c.scale_pairs(ksp, vsp), kd=kd, vd=vd, hv=hv)


@functools.lru_cache(maxsize=None)
def staircase_case8(s, D):
    c = edges.staircase_case(s, D)
    out = dict(q=c["q"], q1=c["q1"], scale=c["scale"], **quantize_case(c["k"], c["v"], s.keys))
    out["hot8"], out["hots"] = k8c.quantize_rows(c["hot"])
    out["hotter8"], out["hotters"] = k8c.quantize_rows(c["hotter"])
    eighth = (out["hotters"].astype(np.float32) / np.float32(8)).astype(np.float16)
    assert np.array_equal(eighth.astype(np.float64) * 8, out["hotters"].astype(np.float64)), "an eighth of the scale is exact"
    out["eighth"] = eighth
    out["ref"], out["absmean"] = ac.prefill_reference(c["q"], out["kd"], out["vd"], s.keys, koff_of(s), c["scale"])
    # the gaps, on the dequantised rows
    q64 = c["q1"].astype(np.float64)
    hotd, hotterd = k8c.dequantize_rows(out["hot8"], out["hots"]), k8c.dequantize_rows(out["hotter8"], out["hotters"])
    s_hot, s_hotter = (q64 * hotd).sum(-1) * c["scale"], (q64 * hotterd).sum(-1) * c["scale"]
    s_decoy = (q64 * k8c.dequantize_rows(out["hotter8"], eighth)).sum(-1) * c["scale"]
    s_rand = ac.scores(c["q1"], out["kd"], c["scale"]).max(-1)
    out["gap"] = float(min((s_hot - s_rand).min(), (s_hotter - s_hot).min()))
    out["gap_scale"] = float((s_hotter - np.maximum(s_decoy, s_rand)).min())
    return out


@functools.lru_cache(maxsize=None)
def pairing_case8(s, D, kind):
    c = edges.pairing_case(s, D, kind)
    out = dict(q=c["q"], pi=c["pi"], scale=c["scale"], **quantize_case(c["k"], c["v"], s.keys))
    out["gap"] = ac.pairing_gap(c["q0"], out["kd"], c["pi"], s.keys, koff_of(s), c["scale"])
    return out


@functools.lru_cache(maxsize=None)
def census_case8(s, D):
    c = edges.census_case(s, D)
    B, Hkv = c["v"].shape[:2]
    v8 = c["v"][:, :, : s.keys].astype(np.int8)
    vs = np.ascontiguousarray(np.broadcast_to(k8c.census_scales(s.keys), (B, Hkv, s.keys)))
    k8, ks = k8c.quantize_rows(c["k"][:, :, : s.keys])
    out = dict(q=c["q"], scale=c["scale"], **from_bytes(k8, ks, v8, vs, s.keys))
    out["ref"], _ = ac.prefill_reference(c["q"], out["kd"], out["vd"], s.keys, koff_of(s), c["scale"])
    return out


@functools.lru_cache(maxsize=None)
def random_case8(s, D, scaling, ramp):
    c = edges.random_case(s, D, scaling, ramp)
    out = dict(q=c["q"], scale=c["scale"], explicit_scale=c["explicit_scale"], **quantize_case(c["k"], c["v"], s.keys))
    out["ref"], out["absmean"] = ac.prefill_reference(c["q"], out["kd"], out["vd"], s.keys, koff_of(s), c["scale"])
    return out


# ---- family drivers: attend(q, k8, v8, sc, keys, koff, scale) -> float16 [B, T, H, D]; koff / scale None = the default --------

def _pairs(B, Hkv):
    return np.repeat(np.arange(B), Hkv), np.tile(np.arange(Hkv), B)


def place(c, placed):
    """copies of (k8, sc) with, for every (rows [B, Hkv], bytes [B, Hkv, D], K scales [B, Hkv]) of `placed`, the row replaced:
    the K scale travels with its bytes; the V side stays"""
    k8, sc = c["k8"].copy(), c["sc"].copy()
    B, Hkv = k8.shape[:2]
    ib, ih = _pairs(B, Hkv)
    for rows, b8, s in placed:
        r = np.asarray(rows).reshape(-1)
        k8[ib, ih, r] = np.asarray(b8).reshape(B * Hkv, -1)
        sc[ib, ih, r, 0] = np.asarray(s).reshape(-1)
    return k8, sc


def check_staircase8(out, c, win):
    """bit equality with fp16(vs * v8) of the winner where there is one, bound8 against the unedited cache's reference elsewhere"""
    B, T, H, D = out.shape
    w = ac.expand_heads(win, H).transpose(0, 2, 1)                                # [B, T, H]
    hv = ac.expand_heads(c["hv"], H)
    exp = hv[np.arange(B)[:, None, None], np.arange(H)[None, None, :], np.maximum(w, 0)]
    exact = w >= 0
    bad = exact & ac.bits_differ(out, exp)
    err = np.abs(out.astype(np.float64) - c["ref"]) / bound8(c["ref"], c["absmean"])
    err = np.where(exact[..., None], 0.0, err)
    bad |= ~exact & ~(err.max(-1) <= 1.0)
    return bad, float(np.nan_to_num(err, nan=np.inf).max()) if err.size else 0.0


def _steps_launch8(attend, s, c, steps):
    """steps: [(rows [B, Hkv], bytes, K scales, rank)]"""
    k8, sc = place(c, [(r, b8, ks) for r, b8, ks, _ in steps])
    out = attend(c["q"], k8, c["v8"], sc, s.keys, s.koff, None)
    assert not np.isnan(out).any(), "NaN in the output"
    win = ac.staircase_winner(s.T, koff_of(s), [(r, rank) for r, _, _, rank in steps])
    return check_staircase8(out, c, win)


def drive_staircase8(attend, s, D):
    """The quantised hot key at the rows around every 32- and 64-key edge, then the two-step variants (edges.step_pairs)."""
    c = staircase_case8(s, D)
    assert c["gap"] >= ac.GAP_MIN, c["gap"]
    heads, worst = s.B * s.Hkv, 0.0
    hot, hotter = (c["hot8"], c["hots"], 1), (c["hotter8"], c["hotters"], 2)
    rows = edges.edge_rows(s.keys)
    for i in range(0, len(rows), heads):
        r = np.resize(np.array(rows[i: i + heads]), heads).reshape(s.B, s.Hkv)
        bad, ratio = _steps_launch8(attend, s, c, [(r,) + hot])
        worst = max(worst, ratio)
        assert not bad.any(), "hot rows %s: %s" % (r.reshape(-1).tolist(), edges._first(bad, "query rows"))
    pairs = edges.step_pairs(s.keys)
    for i in range(0, len(pairs), heads):
        pr = np.resize(np.array(pairs[i: i + heads]), (heads, 2))
        r1, r2 = pr[:, 0].reshape(s.B, s.Hkv), pr[:, 1].reshape(s.B, s.Hkv)
        for first, second, name in ((hot, hotter, "hot then hotter"), (hotter, hot, "hotter then hot")):
            bad, ratio = _steps_launch8(attend, s, c, [(r1,) + first, (r2,) + second])
            worst = max(worst, ratio)
            assert not bad.any(), "%s at %s: %s" % (name, pr.tolist(), edges._first(bad, "query rows"))
    return worst


def drive_by_scale8(attend, s, D):
    """Rows r - 1 and r + 1 carry the hotter key's bytes with an eighth of its K scale: every query that sees row r returns
    fp16(vs[r] * v8[r]) bit for bit (queries that see the decoy r - 1 alone are not judged)."""
    c = staircase_case8(s, D)
    assert c["gap_scale"] >= ac.GAP_MIN, c["gap_scale"]
    heads = s.B * s.Hkv
    rows = [r for r in edges.edge_rows(s.keys) if 1 <= r <= s.keys - 2]
    for i in range(0, len(rows), heads):
        r = np.resize(np.array(rows[i: i + heads]), heads).reshape(s.B, s.Hkv)
        k8, sc = place(c, [(r - 1, c["hotter8"], c["eighth"]), (r + 1, c["hotter8"], c["eighth"]), (r, c["hotter8"], c["hotters"])])
        out = attend(c["q"], k8, c["v8"], sc, s.keys, s.koff, None)
        assert not np.isnan(out).any(), "NaN in the output"
        win = ac.staircase_winner(s.T, koff_of(s), [(r, 1)])
        B, T, H, _ = out.shape
        w = ac.expand_heads(win, H).transpose(0, 2, 1)
        exp = ac.expand_heads(c["hv"], H)[np.arange(B)[:, None, None], np.arange(H)[None, None, :], np.maximum(w, 0)]
        bad = (w >= 0) & ac.bits_differ(out, exp)
        assert not bad.any(), "hot by scale at rows %s: %s" % (r.reshape(-1).tolist(), edges._first(bad, "query rows"))


def drive_pairing8(attend, s, D, kind):
    c = pairing_case8(s, D, kind)
    assert c["gap"] >= ac.GAP_MIN, c["gap"]
    out = attend(c["q"], c["k8"], c["v8"], c["sc"], s.keys, s.koff, None)
    assert not np.isnan(out).any(), "NaN in the output"
    bad = ac.check_pairing(out, dict(pi=c["pi"], v=c["hv"]))
    assert not bad.any(), "%s: %s" % (kind, edges._first(bad, "query rows do not return fp16(vs v8)[pi(t)] bit for bit and are"))


def drive_census8(attend, s, D):
    """vs * v8 is a small multiple of 0.5: every staged value, l = the count and the sum are exact, so the roundings left are
    those of the fp16 census (one fp32 reciprocal, one product, the rounding to fp16)."""
    c = census_case8(s, D)
    out = attend(c["q"], c["k8"], c["v8"], c["sc"], s.keys, s.koff, None)
    assert not np.isnan(out).any(), "NaN in the output"
    err = np.abs(out.astype(np.float64) - c["ref"]) / ac.fp16_ulp(c["ref"])
    empty = ac.prefill_counts(s.T, s.keys, koff_of(s)) == 0
    assert not out[:, empty].any(), "a query with nothing to attend must give zeros"
    bad = ~(err.max(-1) <= 1.0)
    assert not bad.any(), "max error %.3f ulp; %s" % (err.max(), edges._first(bad, "query rows"))
    return float(err.max())


def drive_random8(attend, s, D, scaling, ramp):
    c = random_case8(s, D, scaling, ramp)
    out = attend(c["q"], c["k8"], c["v8"], c["sc"], s.keys, s.koff, c["explicit_scale"])
    assert not np.isnan(out).any(), "NaN in the output"
    ratio = np.abs(out.astype(np.float64) - c["ref"]) / bound8(c["ref"], c["absmean"])
    empty = ac.prefill_counts(s.T, s.keys, koff_of(s)) == 0
    assert not out[:, empty].any(), "a query with nothing to attend must give zeros"
    bad = ~(ratio.max(-1) <= 1.0)
    assert not bad.any(), "max |out - ref| / bound %.3f; %s" % (ratio.max(), edges._first(bad, "query rows"))
    return float(ratio.max())


# ---- the GPU side ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.prefill_attention is None:
        pytest.skip("prefill_attention lives in the compiled module")
    return o


def _len(n):
    return torch.tensor([n], dtype=torch.int64, device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _lay_cache(x, layout):
    """bshd: int8 [B, S, Hkv, D] storage viewed [B, Hkv, S, D]"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if layout != "bshd":
        return t
    B, Hkv, S, D = x.shape
    view = torch.empty((B, S, Hkv, D), dtype=torch.int8, device=DEV).permute(0, 2, 1, 3)
    view.copy_(t)
    assert not view.is_contiguous() and view.stride(2) == Hkv * D
    return view


def _lay_scales(sc, layout):
    """bshd: the scale pairs a view of [B, Hkv, S, 6] storage (the other columns 9.0)"""
    t = torch.from_numpy(np.ascontiguousarray(sc)).to(DEV)
    if layout != "bshd":
        return t
    B, Hkv, S, _ = sc.shape
    view = torch.full((B, Hkv, S, 6), 9.0, dtype=torch.float16, device=DEV)[..., 2:4]
    view.copy_(t)
    assert not view.is_contiguous() and view.stride(2) == 6
    return view


def gpu_attend(ops, layout="plain", splits=None, device_length=False):
    """koff other than keys - T, or device_length: through kv_len = T + koff.  splits forced: once on a NaN-filled and once on
    a zero-filled workspace, the same bits.  splits None here means the unsplit kernel (splits=1), not the rule."""
    def attend(q, k8, v8, sc, keys, koff, scale):
        T = q.shape[1]
        kw = {} if scale is None else {"scaling": scale}
        if device_length or (koff is not None and koff != keys - T):
            n = keys if koff is None else T + koff
            assert 0 <= n <= keys
            kw["kv_len"] = _len(n)
        qd = edges._lay_q(q, "fusedq" if layout == "bshd" else layout)
        kd, vd, sd = _lay_cache(k8, layout), _lay_cache(v8, layout), _lay_scales(sc, layout)
        if splits is None:
            out = ops.prefill_attention_i8kv(qd, kd, vd, sd, keys, splits=1, **kw)
        else:
            outs = []
            for fill in (float("nan"), 0.0):
                ws = torch.full((app.ws_floats(q, splits),), fill, dtype=torch.float32, device=DEV)
                outs.append(ops.prefill_attention_i8kv(qd, kd, vd, sd, keys, splits=splits, workspace=ws, **kw))
            assert _same_bits(outs[0], outs[1]), "the result depends on what the workspace held"
            out = outs[0]
        assert out.shape == q.shape and out.is_contiguous() and out.dtype == torch.float16
        return out.cpu().numpy()
    return attend


def _cases(rows):
    return [(r, i, D, lay) for r in rows for i in range(len(edges.ROWS[r])) for D in DIMS for lay in (("plain", "bshd") if r == 7 else ("plain",))]


def _ids(cases):
    out = []
    for r, i, D, lay in cases:
        s = edges.ROWS[r][i]
        out.append("row%d-T%d-keys%d-koff%s-D%d%s" % (r, s.T, s.keys, "dflt" if s.koff is None else s.koff, D,
                                                       "" if lay == "plain" else "-" + lay))
    return out


STAIRS = _cases((1, 2, 3, 5, 7))
PAIRED = _cases((1, 2, 3, 4, 7))            # pairing needs 0 <= t + koff < keys for every t
EVERY = _cases(TABLE_ROWS)


@pytest.mark.parametrize("row,i,D,layout", STAIRS, ids=_ids(STAIRS))
def test_staircase_block_edges_and_two_steps(ops, row, i, D, layout):
    worst = drive_staircase8(gpu_attend(ops, layout), edges.ROWS[row][i], D)
    print("prefill-i8kv staircase-bait row %d D=%d %s: max ratio %.3f" % (row, D, layout, worst))


@pytest.mark.parametrize("row,i,D,layout", STAIRS, ids=_ids(STAIRS))
def test_hot_by_k_scale_alone(ops, row, i, D, layout):
    drive_by_scale8(gpu_attend(ops, layout), edges.ROWS[row][i], D)


@pytest.mark.parametrize("kind", ("diagonal", "permutation"))
@pytest.mark.parametrize("row,i,D,layout", PAIRED, ids=_ids(PAIRED))
def test_pairing(ops, row, i, D, layout, kind):
    drive_pairing8(gpu_attend(ops, layout), edges.ROWS[row][i], D, kind)


@pytest.mark.parametrize("row,i,D,layout", EVERY, ids=_ids(EVERY))
def test_prefix_census(ops, row, i, D, layout):
    s = edges.ROWS[row][i]
    worst = drive_census8(gpu_attend(ops, layout), s, D)
    print("prefill-i8kv census row %d T=%d koff=%s D=%d %s: max error %.4f ulp" % (row, s.T, s.koff, D, layout, worst))


@pytest.mark.parametrize("scaling,ramp", edges.RANDOM_KINDS, ids=["%s%s" % (a, "-ramp" if b else "") for a, b in edges.RANDOM_KINDS])
@pytest.mark.parametrize("row,i,D,layout", EVERY, ids=_ids(EVERY))
def test_random(ops, row, i, D, layout, scaling, ramp):
    s = edges.ROWS[row][i]
    worst = drive_random8(gpu_attend(ops, layout), s, D, scaling, ramp)
    print("prefill-i8kv random row %d T=%d koff=%s D=%d %s scaling=%s ramp=%d: max ratio %.4f" % (row, s.T, s.koff, D, layout,
                                                                                                 scaling, ramp, worst))


# ---- split ---------------------------------------------------------------------------------------------------------------------

SPLIT, SPLIT_IDS = app.SPLIT, app.SPLIT_IDS
CASES = [(i, D) for i in range(len(SPLIT)) for D in DIMS]
CASE_IDS = ["%s-D%d" % (SPLIT_IDS[i], D) for i, D in CASES]
SPLIT_PAIRED = [(i, D) for i, D in CASES if SPLIT[i][0].koff is None]
SPLIT_PAIRED_IDS = ["%s-D%d" % (SPLIT_IDS[i], D) for i, D in SPLIT_PAIRED]


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_split_staircase_and_scale_across_share_boundaries(ops, i, D):
    s, ns = SPLIT[i]
    worst = drive_staircase8(gpu_attend(ops, splits=ns), s, D)
    drive_by_scale8(gpu_attend(ops, splits=ns), s, D)
    print("prefill-i8kv split staircase-bait %s D=%d: max ratio %.3f" % (SPLIT_IDS[i], D, worst))


@pytest.mark.parametrize("kind", ("diagonal", "permutation"))
@pytest.mark.parametrize("i,D", SPLIT_PAIRED, ids=SPLIT_PAIRED_IDS)
def test_split_pairing(ops, i, D, kind):
    s, ns = SPLIT[i]
    drive_pairing8(gpu_attend(ops, splits=ns), s, D, kind)


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_split_prefix_census(ops, i, D):
    s, ns = SPLIT[i]
    worst = drive_census8(gpu_attend(ops, splits=ns), s, D)
    print("prefill-i8kv split census %s D=%d: max error %.4f ulp" % (SPLIT_IDS[i], D, worst))


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_split_random(ops, i, D):
    s, ns = SPLIT[i]
    worst = max(drive_random8(gpu_attend(ops, splits=ns), s, D, scaling, ramp) for scaling, ramp in edges.RANDOM_KINDS)
    print("prefill-i8kv split random %s D=%d: max ratio %.4f" % (SPLIT_IDS[i], D, worst))


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_default_rule_equals_the_forced_call(ops, i, D):
    """splits=None takes ops.prefill_attention_splits(B, H, T, keys) shares and a workspace of its own."""
    s, _ = SPLIT[i]
    c = random_case8(s, D, "default", False)
    q, k8, v8, sc = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k8", "v8", "sc"))
    n = s.keys if s.koff is None else s.T + s.koff
    rule = ops.prefill_attention_splits(s.B, s.H, s.T, s.keys)
    assert 1 <= rule <= 16
    a = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=_len(n))
    b = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=_len(n), splits=rule)
    assert not torch.isnan(a).any() and _same_bits(a, b)


# ---- device length ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", (1, 3))
@pytest.mark.parametrize("layout", ("plain", "bshd"))
@pytest.mark.parametrize("D", DIMS)
def test_device_length_equals_host_length_bit_for_bit(ops, D, layout, splits):
    """The device-length call against the host-length call (kv_len=None) of the SAME entry with max_keys = the effective keys:
    exact, biased, clamped, Tk < Tq; Tk = 0 and a negative length give zeros."""
    s = app.ROW2
    c = random_case8(s, D, "default", True)
    q = edges._lay_q(c["q"], "fusedq" if layout == "bshd" else layout)
    k8, v8, sc = _lay_cache(c["k8"], layout), _lay_cache(c["v8"], layout), _lay_scales(c["sc"], layout)
    for name, n, bias, keys in app.LENGTHS:
        host = ops.prefill_attention_i8kv(q, k8, v8, sc, keys, splits=splits)
        dev = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=_len(n), kv_len_bias=bias, splits=splits)
        assert not torch.isnan(dev).any(), name
        assert _same_bits(host, dev), name
        if name == "short":
            assert not dev[:, :5].any() and dev[:, 5].any()
    zero = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=_len(9), kv_len_bias=-9, splits=splits)
    assert zero.shape == c["q"].shape and not zero.any() and not torch.isnan(zero).any()
    below = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=_len(-3), splits=splits)
    assert not below.any() and not torch.isnan(below).any()


@pytest.mark.parametrize("D", DIMS)
def test_chunks_equal_the_whole_bit_for_bit(ops, D):
    """Query rows [0, 77), [77, 205), [205, 320) against ONE int8 cache with the counter at 77, 205 and 320 equal the one int8
    call on the whole prompt: every query sees the same quantised rows either way."""
    s = app.ROW1
    c = random_case8(s, D, "default", True)
    q, k8, v8, sc = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k8", "v8", "sc"))
    whole = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys)
    assert not torch.isnan(whole).any()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    for c0, c1 in ((0, 77), (77, 205), (205, 320)):
        counter.fill_(c1)
        part = ops.prefill_attention_i8kv(q[:, c0:c1], k8, v8, sc, s.keys, kv_len=counter)
        assert _same_bits(part, whole[:, c0:c1]), (c0, c1)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(ops):
    s, D = SPLIT[0][0], 64
    c = random_case8(s, D, "default", False)
    q, k8, v8, sc = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k8", "v8", "sc"))
    good = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=_len(s.keys), splits=2)
    with pytest.raises(RuntimeError, match="kv_len"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=torch.tensor([s.keys], dtype=torch.int64))             # on the host
    with pytest.raises(RuntimeError, match="kv_len"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=torch.tensor([s.keys], dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="kv_len_bias"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len_bias=1)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, splits=2,
                                   workspace=torch.zeros(app.ws_floats(c["q"], 2) - 1, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="workspace"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, splits=2,
                                   workspace=torch.zeros(app.ws_floats(c["q"], 2), dtype=torch.float16, device=DEV))
    with pytest.raises(RuntimeError, match="splits"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, splits=0)
    with pytest.raises(RuntimeError, match="splits"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, splits=17)
    with pytest.raises(RuntimeError, match="int8"):
        ops.prefill_attention_i8kv(q, k8.to(torch.float16), v8.to(torch.float16), sc, s.keys)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.prefill_attention_i8kv(q, k8, v8, sc, k8.shape[2] + 1)
    with pytest.raises(RuntimeError, match="8 bytes"):           # a cache whose rows are D + 4 bytes apart: the library refuses
        odd = torch.zeros(k8.shape[:3] + (D + 4,), dtype=torch.int8, device=DEV)[..., :D]
        ops.prefill_attention_i8kv(q, odd, v8, sc, s.keys)
    torch.cuda.synchronize()
    again = ops.prefill_attention_i8kv(q, k8, v8, sc, s.keys, kv_len=_len(s.keys), splits=2)
    assert _same_bits(good, again)
