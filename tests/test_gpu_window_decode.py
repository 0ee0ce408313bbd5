"""The decode kernels with a sliding window (``ops.rope_decode_attention`` / ``ops.decode_attention`` with ``window=W``,
eetq_rope_decode_attention_window_f16 / eetq_decode_attention_window_f16), exact: ``window=W`` must give the BITS of the existing
padded entry called with ``kv_start' = max(s, n - W)`` -- n the row's valid length, the new token included -- in the output and in
the cache rows written; the one-launch and two-launch forms must agree; cache rows below ``kv_start'`` hold NaN and must neither
change nor reach the output.

Shapes: D in {64, 128}, B = 3, 4 / 2 heads, a 1 200-row cache as ONE chunk (the LONG instantiation) and as 5 / 3 chunks (not
LONG), with and without a mask; valid lengths {1, W - 1, W, W + 1, 200, 1 100} for W in {1, 64, 65, 130}; s = None and s with one
row above n - W."""
import numpy as np
import pytest
import torch

import attn_cases as ac
import window_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, HKV, S = 3, 4, 2, 1200
WINDOWS = (1, 64, 65, 130)
# (D, splits): one chunk of 75 / 38 blocks is LONG (more than 16 blocks); 5 x 15 and 3 x 13 blocks are not
CASES = ((128, 1), (128, 5), (64, 1), (64, 3))
CASE_IDS = ["D%d-s%d" % c for c in CASES]


def lengths(W):
    return sorted(set(n for n in (1, W - 1, W, W + 1, 200, 1100) if n >= 1))


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


def _bits(t):
    return t.contiguous().view(torch.int16)


def _i64(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


_inputs = {}


def _decode_inputs(D):
    if D not in _inputs:
        rng = np.random.default_rng(100 + D)
        c = ac.random_case(B, H, HKV, S, D, 7 + D)
        t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
        _inputs[D] = dict(q=t(c["q"]), kc=t(c["k"]), vc=t(c["v"]), k_new=t(ac.normal_f16(rng, (B, HKV, D))),
                          v_new=t(ac.nonzero_normal_f16(rng, (B, HKV, D))), table=t(ac.rope_table(D, 2048)),
                          mask=t(ac.random_mask(B, S + 8, 5 + D)), scale=c["scale"])
    return _inputs[D]


def _one_launch(o, x, D, kc, vc, counter, pos, mask, splits, **kw):
    tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)
    out = o.rope_decode_attention(pos, x["q"], x["k_new"], x["v_new"], x["table"], kc, vc, tickets, slots=counter, mask=mask,
                                  scaling=x["scale"], splits=splits, kv_len=counter, kv_len_bias=1, advance=counter, **kw)
    assert torch.count_nonzero(tickets) == 0, "tickets must be zero between launches"
    return out


def _two_launches(o, x, D, kc, vc, counter, pos, mask, splits, **kw):
    q = x["q"].clone()
    o.rotary_embedding_neox_kvcache(pos, q, x["k_new"].clone(), x["v_new"], D, x["table"], kc, vc, slots=counter)
    return o.decode_attention(q, kc, vc, mask=mask, scaling=x["scale"], splits=splits, kv_len=counter, kv_len_bias=1, advance=counter,
                              **kw)


def _run(o, form, x, D, n, mask, splits, poison_below=None, **kw):
    """one step with n valid rows (the new token, at row n - 1, included) -> (out, kc, vc); poison_below[b]: rows below it hold NaN"""
    kc, vc = x["kc"].clone(), x["vc"].clone()
    if poison_below is not None:
        for b, lo in enumerate(poison_below):
            kc[b, :, :lo] = float("nan")
            vc[b, :, :lo] = float("nan")
    counter = _i64([n - 1])
    out = form(o, x, D, kc, vc, counter, _i64([n - 1] * B), mask, splits, **kw)
    assert int(counter.item()) == n, "the counter advances once"
    return out, kc, vc


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("with_mask", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("D,splits", CASES, ids=CASE_IDS)
def test_window_has_the_bits_of_the_padded_entry(ops, D, splits, with_mask):
    x = _decode_inputs(D)
    mask = x["mask"] if with_mask else None
    for W in WINDOWS:
        for n in lengths(W):
            # s = None, and s with row 0 below, row 1 above and row 2 at n - W
            for s in (None, (max(0, n - W - 5), min(n - 1, max(0, n - W) + 3), max(0, n - W))):
                first = [wc.decode_window_start(n, W, 0 if s is None else s[b]) for b in range(B)]
                kw = {} if s is None else {"kv_start": _i64(list(s))}
                got = {}
                for form in (_one_launch, _two_launches):
                    want = _run(ops, form, x, D, n, mask, splits, kv_start=_i64(first))
                    got[form] = _run(ops, form, x, D, n, mask, splits, window=W, **kw)
                    where = (form.__name__, W, n, s)
                    assert torch.isfinite(want[0]).all() and _same(got[form], want), where
                    # rows below kv_start' are neither read nor written
                    hurt = _run(ops, form, x, D, n, mask, splits, poison_below=first, window=W, **kw)
                    assert torch.isfinite(hurt[0]).all() and torch.equal(_bits(hurt[0]), _bits(want[0])), where
                    for b, lo in enumerate(first):
                        assert torch.isnan(hurt[1][b, :, :lo]).all() and torch.isnan(hurt[2][b, :, :lo]).all(), where
                        assert torch.equal(_bits(hurt[1][b, :, lo:]), _bits(want[1][b, :, lo:])), where
                        assert torch.equal(_bits(hurt[2][b, :, lo:]), _bits(want[2][b, :, lo:])), where
                    if W >= n and s is None:       # the window holds every row: the plain entry
                        assert _same(got[form], _run(ops, form, x, D, n, mask, splits)), where
                assert _same(got[_one_launch], got[_two_launches]), (W, n, s, "the one-launch and two-launch forms must agree")


@pytest.mark.parametrize("with_mask", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("D,splits", CASES, ids=CASE_IDS)
def test_rows_at_different_slots_window_from_their_own_slot(ops, D, splits, with_mask):
    """the one-launch form with a slot per row and no device length: row b's window ends at ITS new token, n_b = slots[b] + 1"""
    x = _decode_inputs(D)
    for W in WINDOWS:
        ns = lengths(W)
        for shift in range(0, len(ns), 2):
            n_b = [ns[(shift + b) % len(ns)] for b in range(B)]
            slots = _i64([n - 1 for n in n_b])
            mask = None
            if with_mask:      # rows beyond a row's slot are masked out, the rest carries the random mask
                mask = x["mask"].clone()
                for b, n in enumerate(n_b):
                    mask[b, n:] = float("-inf")
            for s in (None, (0, min(n_b[1] - 1, max(0, n_b[1] - W) + 3), 1)):
                first = [wc.decode_window_start(n_b[b], W, 0 if s is None else s[b]) for b in range(B)]
                kw = {} if s is None else {"kv_start": _i64(list(s))}
                res = []
                for extra in ({"kv_start": _i64(first)}, dict(window=W, **kw)):
                    kc, vc = x["kc"].clone(), x["vc"].clone()
                    tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)
                    out = ops.rope_decode_attention(slots, x["q"], x["k_new"], x["v_new"], x["table"], kc, vc, tickets, slots=slots,
                                                    mask=mask, scaling=x["scale"], splits=splits, **extra)
                    res.append((out, kc, vc))
                assert torch.isfinite(res[0][0]).all() and _same(res[1], res[0]), (W, n_b, s)
                if with_mask and s is None and W == 1:     # its own token alone (zeros where the mask knocks that column out)
                    alone = x["v_new"].repeat_interleave(H // HKV, dim=1).clone()
                    for b, n in enumerate(n_b):
                        if not torch.isfinite(mask[b, n - 1]):
                            alone[b] = 0
                    assert torch.equal(_bits(res[1][0]), _bits(alone))


@pytest.mark.parametrize("form", (_one_launch, _two_launches), ids=("one", "two"))
def test_window_census(ops, form):
    """q = 0: the mean of the last 65 of 200 small-integer rows (the new token's among them), within 1 fp16 ulp"""
    D, n, W = 64, 200, 65
    v, k = ac.census_values(B, HKV, S, D, seed=9)
    rng = np.random.default_rng(3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    x = dict(q=torch.zeros(B, H, D, dtype=torch.float16, device=DEV), kc=t(k), vc=t(v), k_new=t(ac.normal_f16(rng, (B, HKV, D))),
             v_new=t(v[:, :, n - 1]), table=t(ac.rope_table(D, 2048)), scale=D ** -0.5)
    out, _, _ = _run(ops, form, x, D, n, None, 3, window=W)
    mean = np.repeat(v[:, :, n - W:n].astype(np.float64).mean(axis=2), H // HKV, axis=1)
    err = np.abs(out.cpu().numpy().astype(np.float64) - mean) / ac.fp16_ulp(mean)
    print("decode census: worst error in ulps", float(err.max()))
    assert (err <= 1.0).all(), float(np.nan_to_num(err, nan=np.inf).max())


def test_both_bindings_agree_and_refuse(ops):
    import eetq_amd.ops_ctypes as oc
    D, splits = 128, 5
    x = _decode_inputs(D)
    for W, n in ((64, 200), (130, 1100), (65, 64)):
        for s in (None, (0, max(0, n - W) + 3, 1)):
            kw = {} if s is None else {"kv_start": _i64(list(s))}
            for form in (_one_launch, _two_launches):
                a = _run(ops, form, x, D, n, x["mask"], splits, window=W, **kw)
                b = _run(oc, form, x, D, n, x["mask"], splits, window=W, **kw)
                assert _same(a, b), (form.__name__, W, n, s)
    for o in (ops, oc):
        for bad in (0, -2):
            with pytest.raises(ValueError, match="window must be at least 1"):
                o.decode_attention(x["q"], x["kc"], x["vc"], window=bad)
            with pytest.raises(ValueError, match="window must be at least 1"):
                _one_launch(o, x, D, x["kc"], x["vc"], _i64([3]), _i64([3] * B), None, 1, window=bad)
