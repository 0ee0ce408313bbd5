"""The inputs of tests/test_gpu_act_epilogues.py meet the conditions its assertions rest on (tests/act_cases.py), from the references
alone: the two-hot accumulator is exact in fp32, every wrong order of the epilogue is visible on >= 5 % of a case's elements, the
calibrated gelu bound covers >= 90 % of them -- and every shape of the table selects the kernel form it is listed for on a 256-CU
chip.  No GPU."""
import numpy as np
import pytest

import act_cases as ac

_weights = {}


def _inputs(oracle, case):
    key = (case.K, case.N)
    if key not in _weights:
        _weights.clear()                      # cases are grouped by weight: one at a time
        _weights[key] = ac.weight(case.K, case.N)
    q, s = _weights[key]
    a, b = ac.hot_weights(oracle, q, s, case.M)
    bias, res = ac.bias_residual(case)
    return q, s, a, b, bias, res


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


BY_WEIGHT = sorted(ac.CASES, key=lambda c: (c.K, c.N, c.M, c.id))


@pytest.mark.parametrize("case", BY_WEIGHT, ids=lambda c: c.id)
def test_two_hot_inputs_meet_their_conditions(oracle, case):
    q, s, a, b, bias, res = _inputs(oracle, case)
    k1, k2 = ac.hot_columns(case.M, case.K)
    x = ac.two_hot_x(case.M, case.K)
    assert ((x != 0).sum(1) == 2).all() and (x.sum(1) == 2).all()
    quarter = case.K // 4
    assert (k1 // quarter != k2 // quarter).all()                       # different quarters of K: both slices of any split plan
    assert set(np.unique(q).tolist()) == set(range(-128, 128))
    assert float(s.min()) >= 1e-3 and float(s.max()) <= 2.1e-2
    # (a) the two-weight sum is exact in fp32 for EVERY element -- and is often not an fp16 value, or (b) could not tell the orders apart
    acc = ac.acc_f32(a, b)
    assert np.array_equal(acc.astype(np.float64), a.astype(np.float64) + b.astype(np.float64))
    assert np.isfinite(acc).all() and np.abs(acc).max() < 6.0
    # (b) every mutant differs from the contract (compared as numbers: -0 == +0) on >= 5 % of the elements
    for name, (mutant, want) in ac.relu_mutants(a, b, bias, res).items():
        share = float((mutant.astype(np.float32) != want.astype(np.float32)).mean())
        assert share >= ac.MUTANT_FLOOR, (case.id, name, share)
    # the residual-only launch (bias = None) keeps the order too
    no_bias = ac.relu_contract(a, b, None, res)
    early = np.maximum(acc + res.astype(np.float32), np.float32(0)).astype(np.float16)
    assert float((early.astype(np.float32) != no_bias.astype(np.float32)).mean()) >= ac.MUTANT_FLOOR
    # the calibrated gelu bound applies to >= 90 % of the elements; the allowance itself stays a few ulps
    z = ac.z_f32(a, b, bias)
    assert float((z >= np.float32(ac.GELU_Z_MIN)).mean()) >= ac.GELU_Z_SHARE, case.id
    silu_allow, _ = ac.calibrated_allowance(z, "silu")
    gelu_allow, _ = ac.calibrated_allowance(z, "gelu")
    assert silu_allow.max() <= 2 and gelu_allow[z >= np.float32(ac.GELU_Z_MIN)].max() <= 2, (silu_allow.max(), gelu_allow.max())


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.id)
def test_case_selects_the_form_it_is_listed_for(lib, case):
    ac.check_selection(lib, case)


def test_table_covers_every_listed_form():
    forms = {c.select for c in ac.CASES if c.select[0] in ("stream", "stream_big", "gemv")}
    for want in [("stream", (2, 1, 16)), ("stream", (2, 1, 8)), ("stream", (0, 2, 8)), ("stream", (1, 1, 8)), ("stream", (2, 2, 8)),
                 ("stream", (0, 1, 1)), ("stream", (0, 1, 4)), ("stream_big", (2, 1, 8)), ("stream_big", (2, 2, 8)), ("stream_big", (0, 1, 16))]:
        assert want in forms, want
    assert {c.select[1] for c in ac.GEMV_CASES if c.M == 1} == {"units8", "units884", "k4096_line", "k4096_w8", "generic16", "generic8",
                                                                "shallow8", "shallow4", "shallow1"}
    # the split-K plans: both column-block widths, every slice count, both rings, MT = 1 .. 4, row groups
    plans = [(c.M,) + tuple(c.select[1]) for c in ac.SPLITK_CASES if c.plan]
    assert {p[1] for p in plans} == {1, 2} and {p[2] for p in plans} == {1, 2, 4} and {p[3] for p in plans} == {22, 33}
    assert {(p[0] + 32 * (p[4] if len(p) > 4 else 1) - 1) // (32 * (p[4] if len(p) > 4 else 1)) for p in plans} == {1, 2, 3, 4}
    assert any(len(p) > 4 and p[4] > 1 for p in plans)
    tiles = [t for c in ac.TILED for t in c.select[1]]
    assert {t[0] for t in tiles} == {"wide", "narrow", "stream"}


def test_references_agree_with_the_oracle(oracle):
    """act_f64 on the two-hot z is oracle.w8a16_gemm_bias_act on the two-hot x, bit for bit, and the relu contract is its relu."""
    case = next(c for c in ac.CASES if c.id == "mid-33")
    q, s, a, b, bias, res = _inputs(oracle, case)
    x = ac.two_hot_x(case.M, case.K)
    for bv in (bias, None):
        z = ac.z_f32(a, b, bv)
        for act in ("relu", "silu", "gelu"):
            ref = oracle.w8a16_gemm_bias_act(x, q, s, bv, act)
            assert np.array_equal(ac.act_f64(z, act).view(np.uint16), ref.view(np.uint16)), (act, bv is None)
        assert np.array_equal(ac.relu_contract(a, b, bv).astype(np.float32), oracle.w8a16_gemm_bias_act(x, q, s, bv, "relu").astype(np.float32))


def test_ulp_distance_and_sampling():
    h = np.array([0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 1.0, 1.0 + 2.0 ** -10, -1.0], np.float16)
    assert ac.f16_ordinal(h).tolist()[:4] == [0, 0, 1, -1]
    assert ac.ulp_distance(h[4:5], h[5:6])[0] == 1 and ac.ulp_distance(h[2:3], h[3:4])[0] == 2
    assert ac.ulp_distance(h[4:5], h[6:7])[0] == 2 * 0x3C00
    assert ac.sample_rows(50, 32) == list(range(50))
    assert ac.sample_rows(130, 64) == [0, 31, 32, 63, 64, 65, 127, 128, 129]
    rows = ac.sample_rows(1000, 128)
    assert {0, 31, 32, 500, 999, 127, 128, 895, 896}.issubset(rows) and len(rows) <= 21
    cols = ac.sample_columns(21, 5120, 5120, seams=(4096,))
    assert len(cols) < 600 and {0, 4095, 4096, 5119, 2560}.issubset(cols.tolist())
    assert len(ac.sample_columns(4, 2048, 12320)) == 12320
