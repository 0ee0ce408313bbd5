"""What the assertions of tests/test_gpu_exact_sums.py rest on (tests/exact_cases.py), from the references alone and without a GPU:
every case keeps sum |products| below 2^24 quanta and fp16(q s) exact, with no fp16 subnormal among the operands; the oracle and an
fp32 product taken in three k orders equal the integer reference bit for bit; every mutant -- a lost, doubled or shifted product,
fp16 partial sums, an fp16 running accumulator -- differs from the contract on >= 5 % of a case's elements, while tier A accepts every
early rounding and one lost or doubled product (the quietest of the row) on at least one case (not the two shifts of x against the
weight: their error is of the order of |y| itself, resp. of several whole products, tier A sees them, and they stay as mutants the
exact check must also see); and every shape selects the kernel form it is listed for on a 256-CU chip.  A lost or doubled product of a ZERO activation changes nothing, so those mutants take the nearest k at
which at least half of the rows are non-zero (exact_cases.Problem.loud).

Large cases are analysed on sampled rows (exact_cases.cpu_rows) and, above 2^26 weights, on the first and last columns; the GPU test
asserts the condition on every element of those again."""
import numpy as np
import pytest

import act_cases as ac
import exact_cases as ec

SHIFT = "x_shifted_by_one_k"
SHIFTS = (SHIFT, "last_vector_shifted_by_one_k")
_stats = {}


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def _window(case, w, cols):
    if cols is None:
        return w
    v = ec.Weight.__new__(ec.Weight)
    v.q, v.c4, v.e, v.s = np.ascontiguousarray(w.q[:, cols]), w.c4[cols], w.e[cols], w.s[cols]
    return v


def _analyse(oracle, case):
    """Every per-case assertion; returns {mutant: (share of elements that differ, tier A accepts it)}."""
    if case.id in _stats:
        return _stats[case.id]
    A, c4s, es = ec.level(case)
    stats = {}
    for index in sorted({0, (case.arg or 1) - 1} if case.op == "grouped" else {0}):
        full = ec.Weight(case, index)
        i = ec.activations(case, index)
        rows = ec.cpu_rows(case)
        w = _window(case, full, ec.cpu_cols(case))
        sub = case._replace(N=w.q.shape[1]) if case.op != "gemm_t" else case
        p = ec.Problem(sub, w, i, rows)
        # the inputs: every code, short-mantissa scales, both signs, no subnormal operand
        lo, hi = (-128, 128) if case.bits == 8 else (-8, 8)
        codes = np.flatnonzero(np.bincount(full.q.view(np.uint8).ravel(), minlength=256)).astype(np.uint8).view(np.int8)
        assert set(codes.tolist()) == set(range(lo, hi)), case.id
        assert set(full.c4.tolist()) <= set(c4s) and set(full.e.tolist()) <= set(es) and 6 <= min(es) and max(es) <= ec.E_MAX
        assert np.array_equal(full.s.astype(np.float64), full.c4 / 4.0 * 2.0 ** -full.e)                  # s is c 2^-e exactly
        assert A // 2 < np.abs(i).max() <= A and (i < 0).any() and (i > 0).any(), case.id
        x = ec.as_x(i[rows])
        assert np.array_equal(x.astype(np.float64) * 4, i[rows]) and np.abs(x[x != 0]).min() >= 2.0 ** -14
        # fp16(q s) is exact: the oracle's dequantisation of (q, s) equals q s in float64, and is never subnormal
        kk = np.unique(np.linspace(0, case.K - 1, 256).round().astype(int))
        deq = oracle.dequant(np.ascontiguousarray(w.q[kk]), w.s)
        assert np.array_equal(deq.astype(np.float64), w.q[kk].astype(np.float64) * w.s.astype(np.float64)[None, :]), case.id
        assert np.abs(deq[deq != 0]).min() >= 2.0 ** -9
        # THE CONDITION, from the data
        worst = float(p.bound().max())
        assert worst < ec.LIMIT, (case.id, worst / ec.LIMIT)
        T = p.sums()
        want = p.f16(T)
        assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= 2.0 ** -14).all(), case.id
        # the oracle, bit for bit (on the first rows: about 1e7 of its products)
        if case.op == "gemm_t":
            wd = oracle.dequant(w.q, w.s)
            ref = (x.astype(np.float64) @ wd.astype(np.float64).T).astype(np.float16)       # exact in double: one rounding
            assert np.array_equal(ref.view(np.uint16), (want + np.float16(0)).view(np.uint16)), case.id
            xf, wf = x.astype(np.float32), np.ascontiguousarray(wd.astype(np.float32).T)
        else:
            r = max(1, min(len(rows), int(1e7 // (case.K * sub.N))))
            cc = ac.sample_columns(r, case.K, sub.N)
            ref = oracle.w8a16_gemm(x[:r], np.ascontiguousarray(w.q[:, cc]), np.ascontiguousarray(w.s[cc]))
            assert np.array_equal(ref.astype(np.float32), want[:r][:, cc].astype(np.float32)), case.id
            assert np.array_equal((ref + np.float16(0)).view(np.uint16), (want[:r][:, cc] + np.float16(0)).view(np.uint16)), case.id
            xf, wf = x.astype(np.float32), w.dequant_f64().astype(np.float32)
        # an fp32 product in three k orders holds the exact sum: BLAS's order, k reversed, four interleaved partial sums
        exact = p.f32(T)
        four = xf[:, 0::4] @ wf[0::4]
        for j in (1, 2, 3):
            four = four + xf[:, j::4] @ wf[j::4]
        for name, y in (("forward", xf @ wf), ("reversed", xf[:, ::-1] @ wf[::-1]), ("interleaved", four)):
            assert y.dtype == np.float32 and np.array_equal(y, exact), (case.id, name)
        # the mutants
        for name, y in ec.mutants(p).items():
            share = ec.differs(y, want)
            ok = bool(ac.tier_a(y, want).all())
            old = stats.get(name)
            stats[name] = (share if old is None else min(share, old[0]), ok or bool(old and old[1]))
    _stats[case.id] = stats
    return stats


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.id)
def test_exact_inputs_meet_their_conditions(oracle, case):
    stats = _analyse(oracle, case)
    assert {"lost_first_k", "lost_last_k", "lost_k_at_slice_seam", "doubled_k", "lost_quietest_k", "doubled_quietest_k", *SHIFTS} <= set(stats)
    depth = case.N if case.op == "gemm_t" else case.K
    assert ("fp16_partials_of_2_slices" in stats) == (depth >= 128) and ("fp16_partials_of_4_slices" in stats) == (depth >= 256)
    assert ("fp16_accumulator_every_64_k" in stats) == (depth >= 128)
    for name, (share, _) in stats.items():
        assert share >= ec.MUTANT_FLOOR, (case.id, name, share)


def test_tier_a_accepts_every_mutant_somewhere(oracle):
    """The point of the file: each of these faults passes the |err| <= 1e-3 max|y| + 2e-3 |y| check on some case of the table."""
    accepted = {}
    for case in ec.CASES:
        for name, (_, ok) in _analyse(oracle, case).items():
            accepted.setdefault(name, []).append(case.id) if ok else accepted.setdefault(name, [])
    print({name: len(ids) for name, ids in accepted.items()})
    # Held to it: every early rounding, and ONE lost or doubled product -- the quietest one, since what tier A makes of a single
    # product depends on which one it is (at a fixed k, the first, the last or a seam, it is a matter of luck and not asserted).
    # Not held to it: a shift of the activations against the weight replaces the sum by an uncorrelated one (the whole row) or moves
    # seven products of full size (the last vector), an error of the order of |y| itself resp. of several products against an
    # allowance of 1e-3 max|y|; tier A sees both, and they stay as mutants the exact check must ALSO see (>= 5 % above).
    for name in ("fp16_partials_of_2_slices", "fp16_partials_of_4_slices", "fp16_accumulator_every_64_k", "lost_quietest_k", "doubled_quietest_k"):
        assert accepted[name], name


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.id)
def test_case_selects_the_form_it_is_listed_for(lib, case):
    ec.check_selection(lib, case)


def test_table_covers_every_listed_form():
    by = {f: ec.family(f) for f in ec.FAMILIES}
    # every act_cases shape, under the identity epilogue
    assert {c.id for c in ec.CASES if c.select[0] == "act"} == {c.id for c in ac.CASES}
    # the K-half and slice combines of the tiled kernel
    ids = {c.id for c in by["tiled"]}
    assert {"tile-ragged-round", "guard-tilesplit-256", "guard-auto-128", "tile-shallow-k", "tile-column-split", "tile-wide-act", "tile-narrow-act"} <= ids
    # grouped: both bodies
    assert {b for c in by["grouped"] for b, _ in c.select[1]} == {"w16", "w16_line", "w8"}
    deep = by["deep_k"]
    assert all((c.N if c.op == "gemm_t" else c.K) > 16384 or c.id == "deep-gemv-m4-xv8" for c in deep)
    assert {c.select[1] for c in deep if c.select[0] == "gemv_xv"} == {("units8", 8), ("units884", 8), ("generic16", 4), ("generic8", 8), ("generic16", 8)}
    assert {b for c in deep if c.op == "grouped" for b in c.select[1]} == {("w8", 8), ("w16", 4)}
    assert {c.path for c in deep if c.bits == 8 and c.op == "gemm"} == {"auto", "gemv", "stream", "splitk", "mid", "tilesplit", "mfma"}
    assert {c.select[1][0] for c in deep if c.select[0] == "gemv_i4"} == {"units8", "generic16x4"}
    w4 = by["w4a16"]
    assert {c.select[1][0] for c in w4 if c.select[0] == "gemv_i4"} == {"units8", "k4096_w8", "line32", "line64", "generic16x4", "generic16x2", "shallow8",
                                                                        "shallow4", "shallow1"}
    assert {c.select[1] for c in w4 if c.select[0] == "stream"} == {(2, 1, 16), (2, 1, 8), (2, 2, 8), (2, 2, 16), (0, 2, 16), (0, 1, 8), (0, 2, 8), (1, 1, 8),
                                                                    (0, 1, 4), (0, 1, 1)}
    plans = [c.select[1] for c in w4 if c.select[0] == "splitk_plan"]
    assert {p[0] for p in plans} == {1, 2} and {p[1] for p in plans} == {1, 2, 4} and {p[2] for p in plans} == {22, 33} and any(len(p) > 3 for p in plans)
    assert {c.arg for c in w4 if c.op == "tiled4"} == {0, 1, 2} and any(c.select[0] == "expand" for c in w4)
    for bits in (8, 4):
        grads = [c for c in by["gradient"] if c.bits == bits]
        assert sorted(c.M for c in grads if c.N == 272) == [1, 2, 7, 16, 17, 64, 128, 129, 300] and sorted(c.M for c in grads if c.N == 4096) == [1, 17, 129]
    # every family has a case that also runs through the ctypes binding, where that binding serves it
    assert all(any(c.twin for c in by[f]) for f in ec.FAMILIES)
    # no case is larger than the largest act_cases shape of its form, nor than the deep-K file's
    assert max(c.M * c.K * c.N for c in ec.CASES) == 1024 * 5120 * 5120


def test_mutant_shares_on_the_shapes_the_design_was_checked_at(oracle):
    """(M, K, N) = (5, 4096, 272), (33, 11008, 64), (17, 2048, 272), (4, 16384, 48): two fp16 partials change about a third of the
    outputs, a lost k most of them, and tier A accepts both."""
    for M, K, N in ((5, 4096, 272), (33, 11008, 64), (17, 2048, 272), (4, 16384, 48)):
        case = ec._case("probe", "gemv", M, K, N, "auto", "", ("none", None))
        p = ec.Problem(case, ec.Weight(case), ec.activations(case))
        assert p.bound().max() < ec.LIMIT
        want, m = p.reference(), ec.mutants(p)
        assert ec.differs(m["fp16_partials_of_2_slices"], want) >= 0.2 and ec.differs(m["lost_last_k"], want) >= 0.5, (M, K, N)
        assert ac.tier_a(m["fp16_partials_of_2_slices"], want).all() and ac.tier_a(m["fp16_partials_of_4_slices"], want).all()


def test_the_failure_report_names_a_lost_product():
    """The GPU test's message on a result that lost its last product in one 32-row block and one 16-column block: the count, the blocks,
    the form, and a difference of that product in quanta."""
    from test_gpu_exact_sums import _explain
    case = next(c for c in ec.CASES if c.id == "mid-33")
    w = ec.Weight(case)
    p = ec.Problem(case, w, ec.activations(case))
    want, T = p.reference(), p.sums()
    T[:32, 16:32] -= p.term(p.loud(case.K - 1, -1))[:32, 16:32]
    text = _explain(case, w, p.f16(T), want)
    assert "32-row blocks with wrong elements [0]" in text and "16-column blocks [1] (of 17)" in text and "round-1 tile" in text, text
    assert "mid-33" in text and "first at row" in text and "quanta of" in text
