"""fp32 accumulation and ONE rounding, y = fp16(sum_k fp32(x) fp32(fp16(q s))), in every dense W8A16 / W4A16 kernel form -- bit for
bit, with no tolerance.  The inputs (tests/exact_cases.py) make every product an integer number of quanta and keep the sum of their
magnitudes below 2^24 quanta, so every partial sum in every order is an fp32 value: whatever a kernel's K slices, rings, reduction
trees or MFMA internals, its accumulator holds the exact sum and its result must equal fp16(exact sum) as a number (-0 == +0) on every
element.  A second rounding between the accumulator and the store, or one lost, doubled or misplaced product, changes 5 - 97 % of a
case's elements (tests/test_exact_cases_cpu.py, which also shows tier A accepting those faults, and holds every shape to the kernel
form it is listed for).

The reference is float64 arithmetic on the integers, rounded once on the host; for the large cases the float64 product is formed on
the GPU with torch and checked against NumPy on sampled rows.  The condition (sum |products| < 2^24 quanta) is asserted here on every
element.  One case per family also runs through the ctypes binding.  A failure names the number of wrong elements, the first of them
with both values and their distance in quanta, the 32-row and 16-column blocks that hold wrong elements, and the case's form.

form (family: cases)                                                                                   result on an MI355X
  tiled kernel: wide, narrow, column split, K < 320 chunks, ragged round in 2 K slices,
    K-sliced 128 x 64 tile at 2 / 4 slices, 128 x 128 tile at 2 slices                                      (tiled: 8)        exact
  split-K tile: AUTO + every forced plan -- 1 / 2 / 4 slices, rings 22 / 33, MT = 1 .. 4, row groups        (splitk: 24)      exact
  round-1 tile                                                                                              (mid: 1)          exact
  stream kernel: registers, block copy, 8- / 16- / 32-row rings, two tile rows, shallow forms               (stream: 14)      exact
  GEMV: 8-column and 8 + 8 + 4 units, K = 4096 line, 8-wave forms, generic, shallow, M = 2 .. 4             (gemv: 14)        exact
  grouped GEMV: 16-wave bodies (generic, K = 4096 line), 8-wave body                                        (grouped: 3)      exact
  deep K: XV = 8 GEMV forms, > 64 KiB staging, stream rings, 100+ step slices, int4, grouped, gradients     (deep_k: 36)      exact
  W4A16: GEMV, stream and split-K forms on int4 tiles, the int4 tiled kernel at tile = 0 / 1 / 2, expansion (w4a16: 37)       exact
  input gradient: w8_a16_gemm_t, w4_a16_gemm_t at both tails and at 4096 x 4096                             (gradient: 24)    exact
All 161 cases pass on the device: no kernel or launcher had to change.  Wall time of the file on an MI355X: 10.4 s (the slowest cases:
the first tiled case 1.5 s with the module's start-up, the 40-problem grouped dispatch 1.3 s, every other case under 0.4 s).
"""
import os

import numpy as np
import pytest
import torch

import exact_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ON_DEVICE = 3e8              # above this many products (or 2^25 weights) the float64 reference is formed on the GPU


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as _ops
    from eetq_amd import _lib
    assert _lib.lib().eetq_device_supported() == 1, "kernels are built for gfx950 only"
    return _ops


@pytest.fixture(scope="module")
def weights():
    """{(bits, gradient?, K, N): {index: (Weight, packed on the GPU, scales on the GPU)}}: one shape at a time, dropped with the module"""
    cache = {}
    yield cache
    cache.clear()


def _weight(ops, oracle, weights, case, index=0):
    key = (case.bits, case.op == "gemm_t", case.K, case.N)
    if key not in weights:
        weights.clear()
        torch.cuda.empty_cache()
        weights[key] = {}
    if index not in weights[key]:
        w = ec.Weight(case, index)
        raw = w.q if case.bits == 8 else oracle.i4_from_values(w.q)
        if w.q.size <= 1 << 25:
            packed = torch.from_numpy(oracle.gfx950_pack(raw) if case.bits == 8 else oracle.gfx950_pack_i4(raw)).to(DEV)
        else:                    # a large weight: packed on the device (bit-exact against the oracle in test_gpu_parity.py / test_gpu_int4.py)
            packed = ops.preprocess_weights(torch.from_numpy(raw).to(DEV), case.bits == 4)
        weights[key][index] = (w, packed, torch.from_numpy(w.s).to(DEV))
    return weights[key][index]


def _needs_256_cus():
    if torch.cuda.get_device_properties(0).multi_processor_count != ec.NCU:
        pytest.skip("the shapes select their kernel forms on a 256-CU chip")


def _binding(ops, case, twin):
    if twin:
        from eetq_amd import ops_ctypes
        return ops_ctypes
    if case.bits == 4 and case.op == "gemm" and ops.BOUNDARY != "ext":
        pytest.skip("int4 goes through the compiled module (EETQ_AMD_BOUNDARY=ctypes selects the twin binding)")
    return ops


def _launch(b, case, x, packed, s):
    """One launch on the case's path; a split-K plan is forced in-process for exactly this launch."""
    if case.op == "gemm_t":
        return (b.w8_a16_gemm_t if case.bits == 8 else b.w4_a16_gemm_t)(x, packed, s)
    if case.op == "tiled4":
        return b.w4_a16_gemm_tiled(x, packed, s, tile=case.arg)
    if case.plan:
        os.environ["EETQ_AMD_SPLITK_PLAN"] = case.plan
    try:
        y = b.w8_a16_gemm(x, packed, s, path=case.path)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("EETQ_AMD_SPLITK_PLAN", None)
    return y


def _reference(case, w, i):
    """(fp16 reference, largest sum of |products| in quanta) over every element"""
    if case.M * case.K * case.N <= ON_DEVICE and w.q.size <= 1 << 25:
        p = ec.Problem(case, w, i)
        return p.reference(), float(p.bound().max())
    if case.op == "gemm_t":      # exact_cases.Problem: the reduction runs over n, the scales' powers of two inside it
        a = torch.from_numpy(i.astype(np.int64) * (w.c4 * 2 ** (ec.E_MAX - w.e))[None, :]).to(DEV).double()
        b, col = torch.from_numpy(w.q).to(DEV).double().t(), torch.ones(case.K, dtype=torch.float64, device=DEV)
    else:
        a, b = torch.from_numpy(i).to(DEV).double(), torch.from_numpy(w.q).to(DEV).double()
        col = torch.from_numpy(w.c4).to(DEV).double()
    T = ((a @ b) * col[None, :]).cpu().numpy()                   # integers far below 2^53: exact in any order
    bound = float(((a.abs() @ b.abs()) * col[None, :]).max())
    del a, b
    want = (T * ec.quantum(case, w)[None, :]).astype(np.float16)  # ONE rounding, float64 -> fp16, on the host
    rows, cols = ec.cpu_rows(case), ec.cpu_cols(case)
    spot = ec.Problem(case, w, i, rows, cols).reference()
    assert np.array_equal(spot, want[rows] if cols is None else want[rows][:, cols]), "the device-side reference disagrees with NumPy"
    return want, bound


def _explain(case, w, got, want):
    bad = np.argwhere(got.astype(np.float32) != want.astype(np.float32))
    m, n = bad[0]
    dq = ec.quanta_between(case, w, got, want)
    vals, counts = np.unique(np.round(dq[bad[:, 0], bad[:, 1]], 2), return_counts=True)
    top = [(float(vals[j]), int(counts[j])) for j in np.argsort(-counts)[:6]]
    return ("%s [%s]: %d of %d elements differ from fp16(exact sum); first at row %d column %d: device %r, reference %r, %+.2f quanta of %g; "
            "32-row blocks with wrong elements %s, 16-column blocks %s (of %d); commonest differences in quanta (value, count) %s"
            % (case.id, case.form, len(bad), got.size, m, n, float(got[m, n]), float(want[m, n]), dq[m, n], ec.quantum(case, w)[n],
               sorted(set((bad[:, 0] // 32).tolist()))[:12], sorted(set((bad[:, 1] // 16).tolist()))[:12], (got.shape[1] + 15) // 16, top))


def _check(case, w, got, want, bound):
    assert bound < ec.LIMIT, (case.id, bound / ec.LIMIT)
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float16, case.id
    if not np.array_equal(got.astype(np.float32), want.astype(np.float32)):
        pytest.fail(_explain(case, w, got, want))


def _run(ops, oracle, weights, case):
    _needs_256_cus()
    b = _binding(ops, case, False)
    if case.op == "grouped":
        probs = [_weight(ops, oracle, weights, case, j) for j in range(case.arg)]
        acts = [ec.activations(case, j) for j in range(case.arg)]
        xs = [torch.from_numpy(ec.as_x(i)).to(DEV) for i in acts]
        outs = b.w8_a16_gemv_grouped(xs, [p[1] for p in probs], [p[2] for p in probs])
        twin = _binding(ops, case, True).w8_a16_gemv_grouped(xs, [p[1] for p in probs], [p[2] for p in probs]) if case.twin else None
        assert len(outs) == case.arg
        for j, ((w, _, _), i) in enumerate(zip(probs, acts)):
            want, bound = _reference(case, w, i)
            _check(case._replace(id="%s, problem %d" % (case.id, j)), w, outs[j], want, bound)
            if twin is not None:
                _check(case._replace(id="%s, problem %d, ctypes binding" % (case.id, j)), w, twin[j], want, bound)
        return
    w, packed, s = _weight(ops, oracle, weights, case)
    i = ec.activations(case)
    x = torch.from_numpy(ec.as_x(i)).to(DEV)
    want, bound = _reference(case, w, i)
    _check(case, w, _launch(b, case, x, packed, s), want, bound)
    if case.twin:
        _check(case._replace(id=case.id + ", ctypes binding"), w, _launch(_binding(ops, case, True), case, x, packed, s), want, bound)


def _by_weight(name):
    return sorted(ec.family(name), key=lambda c: (c.bits, c.op == "gemm_t", c.K, c.N, c.M, c.id))


@pytest.mark.parametrize("case", _by_weight("tiled"), ids=lambda c: c.id)
def test_tiled_kernel(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("splitk"), ids=lambda c: c.id)
def test_splitk_tile(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("mid"), ids=lambda c: c.id)
def test_round_1_tile(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("stream"), ids=lambda c: c.id)
def test_stream_kernel(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("gemv"), ids=lambda c: c.id)
def test_gemv(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("grouped"), ids=lambda c: c.id)
def test_grouped_gemv(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("deep_k"), ids=lambda c: c.id)
def test_deep_k(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("w4a16"), ids=lambda c: c.id)
def test_w4a16(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)


@pytest.mark.parametrize("case", _by_weight("gradient"), ids=lambda c: c.id)
def test_input_gradient(ops, oracle, weights, case):
    _run(ops, oracle, weights, case)

