"""The MFMA prompt kernel with a sliding window (``ops.prefill_attention(..., window=W)``, eetq_prefill_attention_window_f16): a
query at cache row p attends rows max(0, p - W + 1) .. p.

Shapes (window_cases.py): D in {64, 128}, B = 2, 4 / 2 heads; a fresh prompt of 160 rows (two query blocks, the second ragged)
and 40 rows behind 260 cached ones through a device ``kv_len``, unsplit and with 2 and 4 shares; W in {1, 5, 64, 65, 129, keys,
keys + 7}.  Exact wherever the arithmetic allows it: W = 1 returns the row's own V, the oldest-wins staircase returns V of the
oldest hot row inside the window (a key leaked from just below the window is older, hence hotter, and wins), W >= keys and every
row with t + koff < W have the plain entry's bits."""
import functools

import numpy as np
import pytest
import torch

import attn_cases as ac
import window_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (name, shape, length on the device, splits)
FORMS = (("fresh", "fresh", False, 1), ("fresh_s2", "fresh", False, 2), ("behind", "behind", True, 1), ("behind_s2", "behind", True, 2),
         ("behind_s4", "behind", True, 4))
FORM_IDS = [f[0] for f in FORMS]


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.prefill_attention is None:
        pytest.skip("prefill_attention lives in the compiled module")
    return o


def _bits(t):
    return t.contiguous().view(torch.int16)


def _dev(*xs):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs)


def _call(ops, q, k, v, keys, on_device, splits, **kw):
    if on_device:
        kw["kv_len"] = torch.tensor([keys], dtype=torch.int64, device=DEV)
    return ops.prefill_attention(q, k, v, keys, splits=splits, **kw)


@functools.lru_cache(maxsize=None)
def _random(shape, D):
    T, keys = wc.SHAPES[shape]
    return ac.prefill_random_case(wc.B, T, wc.H, wc.HKV, keys, D, seed=17 * D + keys)


@functools.lru_cache(maxsize=None)
def _random_ref(shape, D, W):
    c = _random(shape, D)
    T, keys = wc.SHAPES[shape]
    return wc.window_reference(c["q"], c["k"], c["v"], keys, keys - T, W, c["scale"])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("D", wc.DIMS)
def test_window_of_one_returns_the_rows_own_value(ops, D, form):
    _, shape, on_device, splits = form
    T, keys = wc.SHAPES[shape]
    c = _random(shape, D)
    q, k, v = _dev(c["q"], c["k"], c["v"])
    out = _call(ops, q, k, v, keys, on_device, splits, window=1, scaling=c["scale"])
    want = v[:, :, keys - T:keys].repeat_interleave(wc.H // wc.HKV, dim=1).transpose(1, 2)     # [B, T, H, D]
    assert out.shape == (wc.B, T, wc.H, D) and torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("D", wc.DIMS)
def test_oldest_hot_row_inside_the_window_wins(ops, D, form):
    _, shape, on_device, splits = form
    c = wc.staircase_case(shape, D, seed=11 + D)
    assert wc.staircase_gap(c) >= ac.GAP_MIN
    T, keys, koff = c["T"], c["keys"], c["koff"]
    q, k, v = _dev(c["q"], c["k"], c["v"])
    for W in wc.windows(keys):
        out = _call(ops, q, k, v, keys, on_device, splits, window=W, scaling=c["scale"]).cpu().numpy()
        ref, absmean = wc.window_reference(c["q"], c["k"], c["v"], keys, koff, W, c["scale"])
        bad, win = wc.check_window_staircase(out, c, W, ref, absmean)
        assert not bad.any(), (form[0], D, W, "queries", sorted(set(np.argwhere(bad)[:, 1].tolist()))[:12], "winners", win[:8])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("D", wc.DIMS)
def test_window_census(ops, D, form):
    _, shape, on_device, splits = form
    c = wc.census_case(shape, D, seed=5 + D)
    T, keys, koff = c["T"], c["keys"], c["koff"]
    q, k, v = _dev(c["q"], c["k"], c["v"])
    for W in wc.windows(keys):
        out = _call(ops, q, k, v, keys, on_device, splits, window=W, scaling=c["scale"]).cpu().numpy().astype(np.float64)
        mean = np.repeat(wc.window_census_mean(c["v"], T, keys, koff, W), wc.H // wc.HKV, axis=2)
        err = np.abs(out - mean) / ac.fp16_ulp(mean)
        print("census", form[0], D, W, "worst error in ulps", float(err.max()))
        assert (err <= 1.0).all(), (form[0], D, W, float(np.nan_to_num(err, nan=np.inf).max()))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("D", wc.DIMS)
def test_wide_windows_and_early_rows_have_the_plain_bits(ops, D, form):
    _, shape, on_device, splits = form
    T, keys = wc.SHAPES[shape]
    koff = keys - T
    c = _random(shape, D)
    q, k, v = _dev(c["q"], c["k"], c["v"])
    plain = _call(ops, q, k, v, keys, on_device, splits, scaling=c["scale"])
    assert torch.isfinite(plain).all()
    if not on_device and splits == 1:     # the fresh prompt's host form has the same bits
        assert torch.equal(_bits(plain), _bits(ops.prefill_attention(q, k, v, keys, scaling=c["scale"])))
    for W in wc.windows(keys):
        out = _call(ops, q, k, v, keys, on_device, splits, window=W, scaling=c["scale"])
        early = max(0, min(T, W - koff))      # rows with t + koff < W
        assert W < keys or early == T
        assert torch.equal(_bits(out[:, :early]), _bits(plain[:, :early])), (form[0], D, W, early)
        if 1 < W < keys:                      # ... and the window does change the later rows
            assert not torch.equal(_bits(out[:, early:]), _bits(plain[:, early:])), (form[0], D, W)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("D", wc.DIMS)
def test_random_data_against_the_windowed_reference(ops, D, form):
    _, shape, on_device, splits = form
    T, keys = wc.SHAPES[shape]
    c = _random(shape, D)
    q, k, v = _dev(c["q"], c["k"], c["v"])
    for W in wc.windows(keys):
        out = _call(ops, q, k, v, keys, on_device, splits, window=W, scaling=c["scale"]).cpu().numpy().astype(np.float64)
        ref, absmean = _random_ref(shape, D, W)
        ratio = np.abs(out - ref) / ac.random_bound(ref, absmean)
        print("random", form[0], D, W, "worst error / bound", float(ratio.max()))
        assert (ratio <= 1.0).all(), (form[0], D, W, float(np.nan_to_num(ratio, nan=np.inf).max()))


@pytest.mark.parametrize("splits", (1, 2, 4))
@pytest.mark.parametrize("D", wc.DIMS)
def test_rows_below_the_first_needed_block_are_never_read(ops, D, splits):
    T, keys = wc.SHAPES["behind"]
    W, koff = 65, keys - T
    floor = 64 * (max(0, koff - W + 1) // 64)
    assert floor == 192
    c = _random("behind", D)
    q, k, v = _dev(c["q"], c["k"], c["v"])
    want = _call(ops, q, k, v, keys, True, splits, window=W, scaling=c["scale"])
    kn, vn = k.clone(), v.clone()
    for t in (kn, vn):
        t[:, :, :floor] = float("nan")
        assert torch.isnan(t[:, :, keys:]).all()       # the generator's own poison beyond the keys
    out = _call(ops, q, kn, vn, keys, True, splits, window=W, scaling=c["scale"])
    assert torch.isfinite(out).all() and torch.equal(_bits(out), _bits(want))


def test_refusals(ops):
    c = _random("fresh", 64)
    T, keys = wc.SHAPES["fresh"]
    q, k, v = _dev(c["q"], c["k"], c["v"])
    for bad in (0, -4):
        with pytest.raises(ValueError, match="window must be at least 1"):
            ops.prefill_attention(q, k, v, keys, window=bad)
    with pytest.raises(ValueError, match="window and kv_start"):
        ops.prefill_attention(q, k, v, keys, window=8, kv_start=torch.zeros(wc.B, dtype=torch.int64, device=DEV))
    k8 = torch.zeros(wc.B, wc.HKV, keys, 64, dtype=torch.int8, device=DEV)
    sc = torch.ones(wc.B, wc.HKV, keys, 2, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="no sliding window on int8 rows"):
        ops.prefill_attention_i8kv(q, k8, k8.clone(), sc, keys, window=8)
    assert torch.isfinite(ops.prefill_attention_i8kv(q, k8, k8.clone(), sc, keys)).all()      # ... and is as it was without one
    with pytest.raises(RuntimeError, match="causal_offset"):
        ops.prefill_attention(q, k, v, keys, causal_offset=3, window=8)
