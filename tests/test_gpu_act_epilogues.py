"""The bias + activation epilogue, y = fp16(act(acc + fp32(bias[n]))) [+ residual, an fp16 add], in every forward W8A16 kernel form
that compiles it (common.hpp::finish_element / finish_quad): the GEMV forms, the stream kernel's register and LDS forms, the round-1
tile, the split-K tile on every plan, both ACT instantiations of the tiled kernel, column-split launches, and the launches that an
activation sends to another kernel than the identity epilogue (tests/act_cases.py has the table and says why each shape selects its
form; tests/test_act_cases_cpu.py checks that, and the conditions the exact checks rest on, without a GPU).

Per case: (1) relu on two-hot rows equals the float32 contract EXACTLY, with bias, bias + residual and residual only -- which tells
fp16(act(acc + bias)) from act(fp16(acc) + bias), from a residual added before the activation, and from a bias read a few columns
over; (2) silu and gelu on the same rows within a bound calibrated from two references; (3) tier A against the oracle on random
rows; (4) two launches give the same bits; (5) the same bits as the twin kernel where one exists.

Measured on an MI355X, two-hot rows, distance of the device's result from the double reference in fp16 ulps (largest over the
calibrated elements | share of them that differ at all), per kernel form -- the allowance is 1 + the float32-vs-double distance:

  form (cases)                                                   silu               gelu (z >= -3)
  tiled ACT tiles, wide / narrow / column split / ragged round   1 | 1.5e-5..3.5e-5  1 | 7.6e-5..1.9e-4
  tiled path at K < 320 (stream kernel, 64-row chunks)           1 | 5.7e-5          1 | 1.7e-4
  tilesplit / AUTO / mfma at M = 256; activated AUTO at M = 128  1 | 1.5e-5..4.6e-5  1 | 1.5e-4..2.0e-4
  split-K tile, M = 17 (AUTO and five forced plans)              0 | 0               0 | 0
  split-K tile, M = 50 / 100 / 128 (every forced plan)           0 | 0               1 | 1.5e-4..2.4e-4
  split-K tile, M = 80 (MT = 3)                                  1 | 4.6e-5          1 | 1.9e-4
  round-1 tile, M = 33                                           0 | 0               1 | 3.4e-4
  stream, N = 272: 8- / 16-row rings (M = 5, 9, 12), M = 40      0 | 0               0 | 0
  stream, N = 272: 16-row ring M = 16, 32-row ring M = 17 / 32   0 | 0               1 | 2.3e-4..4.4e-4
  stream, two tile rows (regs, 8- / 16- / 32-row rings)          1 | 1.0e-5..8.1e-5  1 | 1.3e-4..3.3e-4
  stream, block copy                                             0 | 0               1 | 3.3e-4
  stream, shallow one-wave / four-wave forms                     0 | 0               1 | 7.5e-4 / 0 | 0
  GEMV M = 1: 8-column units, K = 4096 straight-line, 16-wave
    generic, shallow K = 1024 / 64                               0 | 0               0 | 0
  GEMV M = 1: 8 + 8 + 4 units, both 8-wave forms                 0 | 0               1 | 1.2e-4..2.0e-4
  GEMV M = 1 shallow K = 256 (272 elements)                      0 | 0               1 | 3.7e-3
  GEMV M = 2 .. 4                                                0 | 0               0..1 | 0..9.5e-4
The epilogue's arithmetic depends on z alone, so the differences between forms are differences between their inputs: no element of any
form is further than one fp16 ulp from the double reference, at most 8e-5 of a case's elements differ under silu and 4e-3 under gelu.
Every case passes on the device; no kernel or launcher had to change.
"""
import os

import numpy as np
import pytest
import torch

import act_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = ("relu", "gelu", "silu")


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as _ops
    from eetq_amd import _lib
    assert _lib.lib().eetq_device_supported() == 1, "kernels are built for gfx950 only"
    return _ops


@pytest.fixture(scope="module")
def weights():
    """(K, N) -> (q, s, packed on the GPU, scales on the GPU); shared by the cases of a shape, dropped with the module."""
    cache = {}
    yield cache
    cache.clear()


def _weight(oracle, weights, K, N):
    if (K, N) not in weights:
        q, s = ac.weight(K, N)
        weights[(K, N)] = (q, s, torch.from_numpy(oracle.gfx950_pack(q)).to(DEV), torch.from_numpy(s).to(DEV))
    return weights[(K, N)]


def _needs_256_cus():
    if torch.cuda.get_device_properties(0).multi_processor_count != ac.NCU:
        pytest.skip("the shapes select their kernel forms on a 256-CU chip")


def _launch(ops, case, x, w, s, path=None, **kw):
    """One launch on the case's path; the split-K plan is forced in-process for exactly this launch."""
    if case.plan and path is None:
        os.environ["EETQ_AMD_SPLITK_PLAN"] = case.plan
    try:
        y = ops.w8_a16_gemm(x, w, s, path=path or case.path, **kw)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("EETQ_AMD_SPLITK_PLAN", None)
    return y


def _same(got, want):
    """Equal as numbers (-0 == +0), every element."""
    return np.array_equal(got.astype(np.float32), want.astype(np.float32))


def _where(got, want):
    bad = np.argwhere(got.astype(np.float32) != want.astype(np.float32))
    m, n = bad[0]
    return "%d of %d differ; first at row %d column %d: got %r want %r" % (len(bad), got.size, m, n, float(got[m, n]), float(want[m, n]))


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.id)
def test_two_hot_rows(ops, oracle, weights, case):
    """Checks 1 and 2 on the two-hot rows."""
    _needs_256_cus()
    q, s, wd, sd = _weight(oracle, weights, case.K, case.N)
    a, b = ac.hot_weights(oracle, q, s, case.M)
    bias, res = ac.bias_residual(case)
    xd = torch.from_numpy(ac.two_hot_x(case.M, case.K)).to(DEV)
    bd, rd = torch.from_numpy(bias).to(DEV), torch.from_numpy(res).to(DEV)
    # 1. relu, exact: bias; bias + residual; residual only
    for name, kw, want in (("bias", dict(bias=bd), ac.relu_contract(a, b, bias)),
                           ("bias + residual", dict(bias=bd, residual=rd), ac.relu_contract(a, b, bias, res)),
                           ("residual only", dict(residual=rd), ac.relu_contract(a, b, None, res))):
        got = _launch(ops, case, xd, wd, sd, activation="relu", **kw).cpu().numpy()
        assert got.shape == want.shape
        assert _same(got, want), "%s, relu, %s: %s" % (case.id, name, _where(got, want))
    # 2. silu and gelu against the double reference, within the distance of the float32 reference from it plus one fp16 ulp
    z = ac.z_f32(a, b, bias)
    for act in ("silu", "gelu"):
        got = _launch(ops, case, xd, wd, sd, activation=act, bias=bd).cpu().numpy()
        ok, worst, share = ac.check_calibrated(got, z, act)
        print("ACTFIG %s | %s | %s | max %d ulp | differing %.3e" % (case.id, case.form, act, worst, share))
        if not ok.all():
            m, n = np.argwhere(~ok)[0]
            allow, ref = ac.calibrated_allowance(z, act)
            pytest.fail("%s, %s: %d of %d outside the bound; first at row %d column %d: z = %r, device %r, double reference %r, float32 "
                        "reference %r, allowance %d ulp" % (case.id, act, int((~ok).sum()), ok.size, m, n, float(z[m, n]), float(got[m, n]),
                                                            float(ref[m, n]), float(ac.act_f32(z, act)[m, n]), int(allow[m, n])))
        # the residual is an fp16 add after the activation
        got_res = _launch(ops, case, xd, wd, sd, activation=act, bias=bd, residual=rd).cpu().numpy()
        assert _same(got_res, got + res), "%s, %s + residual: %s" % (case.id, act, _where(got_res, got + res))


def _seams(case):
    return [t[1] for t in case.select[1][1:]] if case.select[0] == "mfma" and case.select[1][0][0] != "stream" else []


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.id)
def test_random_rows(ops, oracle, weights, case):
    """Checks 3, 4 and 5 on random activations of both signs."""
    _needs_256_cus()
    q, s, wd, sd = _weight(oracle, weights, case.K, case.N)
    bias, res = ac.bias_residual(case)
    x = ac.random_x(case)
    xd, bd, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(bias).to(DEV), torch.from_numpy(res).to(DEV)
    rows = ac.sample_rows(case.M, ac.row_group(case))
    cols = ac.sample_columns(len(rows), case.K, case.N, _seams(case))
    xr, qc, sc, bc = x[rows], np.ascontiguousarray(q[:, cols]), np.ascontiguousarray(s[cols]), np.ascontiguousarray(bias[cols])
    outs = {}
    for act in ACTS:
        y = _launch(ops, case, xd, wd, sd, activation=act, bias=bd)
        outs[act] = y
        got = y.cpu().numpy()[np.ix_(rows, cols)]
        ref = oracle.w8a16_gemm_bias_act(xr, qc, sc, bc, act)
        ok = ac.tier_a(got, ref)
        assert ok.all(), (case.id, act, int((~ok).sum()), float(np.abs(got.astype(np.float32) - ref.astype(np.float32)).max()))
    if case.id == "guard-auto-128":   # what act == 0 decides: the identity launch of this shape is the K-sliced tiled kernel
        from eetq_amd import _lib
        assert ac.auto_path(_lib.lib(), case.M, case.N, case.K) == (ac.TILESPLIT, 4)
    # 4. two launches, the same bits (fused residual included)
    for act in ACTS:
        assert torch.equal(_launch(ops, case, xd, wd, sd, activation=act, bias=bd), outs[act]), (case.id, act)
    yr1 = _launch(ops, case, xd, wd, sd, activation="gelu", bias=bd, residual=rd)
    yr2 = _launch(ops, case, xd, wd, sd, activation="gelu", bias=bd, residual=rd)
    assert torch.equal(yr1, yr2) and torch.equal(yr1, outs["gelu"] + rd), case.id
    # 5. twins
    if case.twin == "subproblem":
        # the second launch of a column split is the narrow ACT tile on columns c0 .. N with every pointer moved by c0: the same
        # bits as that kernel launched on those columns alone
        (_, c0, n1) = case.select[1][1]
        assert ac.mfma_launches(case.M, n1, case.K) == [("narrow", 0, n1)]
        w1 = torch.from_numpy(oracle.gfx950_pack(np.ascontiguousarray(q[:, c0:]))).to(DEV)
        for act in ACTS:
            alone = ops.w8_a16_gemm(xd, w1, sd[c0:].contiguous(), path="mfma", bias=bd[c0:].contiguous(), residual=rd[:, c0:].contiguous(),
                                    activation=act)
            assert torch.equal((outs[act] + rd)[:, c0:], alone), (case.id, act)
    elif case.twin:
        for path in case.twin.split(","):
            for act in ACTS:
                assert torch.equal(_launch(ops, case, xd, wd, sd, path=path, activation=act, bias=bd), outs[act]), (case.id, path, act)
