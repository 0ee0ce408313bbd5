"""What the assertions of tests/test_gpu_moe_exact.py rest on (tests/moe_exact_cases.py), from the references alone and without a GPU:
the routing table is the one the cases are listed for; every K of the decode kernel selects, by the restated plan rule, the (waves,
depth) and the tiles per wave it is listed for, and the table shows every feature of the K loop each instantiation can show (r = 0 and
r = 1 where D = 2, waves with unequal tile counts, the steady loop running and not running); every expert of every case keeps sum
|products| below 2^24 quanta on every element; the oracle and an fp32 product in three k orders equal the integer reference bit for
bit; every mutant differs from the reference on >= 5 % of the elements of the rows it touches; and which mutants tier A (|err| <=
1e-3 max|ref| + 2e-3 |ref| per expert, untouched rows past offsets[E]) accepts -- printed, and asserted as seen here.

Tier A on these inputs, as seen here (decode: 19 cases, the number is the cases on which the tier-A tests would have passed):
  fp16_partials_of_2_slices 18, fp16_partials_of_4_slices 17, fp16_wave_partials 16, fp16_accumulator_every_64_k 14: every early
      rounding is accepted nearly everywhere;
  ONE lost or doubled product, the quietest: accepted on 8 cases (int4 from K = 384 on) where one row decides what quiet is (the 1-row
      expert), on none on the 33-row expert (over 33 rows and 48 columns every k holds a large |x| and a large |q s| somewhere, and K
      stays below 9088: the dense table's deep-K cases are where tier A accepts it on many rows);
  rejected on every case: a lost or doubled k TILE of one wave (64 or 128 products), the next expert's weight or scales, the slot's
      row of x in place of the token's, the clamped row stored one past, the two shifts of x, a product at a fixed k (first, last,
      seam, K / 3: these four are a matter of luck and are not asserted).
  combine (48 cases): products_rounded_to_fp16 32, fp16_accumulator 32 (every case with k > 1); a dropped slot and a neighbour's
      weight on none.
So tier A would have seen a lost tile HAD IT RUN these K; what it cannot see at any K is the early rounding and the single product."""
import numpy as np
import pytest

import act_cases as ac
import exact_cases as ec
import moe_exact_cases as mc

_stats = {}


def _three_orders(p, x, wf):
    """BLAS's order, k reversed, four interleaved partial sums: all hold the exact sum"""
    exact = p.f32(p.sums())
    xf = x.astype(np.float32)
    four = xf[:, 0::4] @ wf[0::4]
    for j in (1, 2, 3):
        four = four + xf[:, j::4] @ wf[j::4]
    for name, y in (("forward", xf @ wf), ("reversed", xf[:, ::-1] @ wf[::-1]), ("interleaved", four)):
        assert y.dtype == np.float32 and np.array_equal(y, exact), (p.case.id, name)


def _check_routed(oracle, rp):
    """the condition and the reference of every live expert"""
    case = rp.case
    for e, p in rp.p.items():
        w = rp.w[e]
        worst = float(p.bound().max())
        assert worst < mc.LIMIT, (case.id, e, worst / mc.LIMIT)
        want = p.reference()
        assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= 2.0 ** -14).all(), (case.id, e)
        x = mc.as_x(rp.i[rp.rows(e)])
        deq = w.dequant_f64()
        assert np.array_equal(oracle.dequant(w.q, w.s).astype(np.float64), deq), (case.id, e)      # fp16(q s) is exact
        if case.op == "gemm_t":
            ref = (x.astype(np.float64) @ deq.T).astype(np.float16)                                 # exact in double: one rounding
            assert np.array_equal(ref.astype(np.float32), want.astype(np.float32)), (case.id, e)
            _three_orders(p, x, np.ascontiguousarray(deq.T.astype(np.float32)))
        else:
            ref = oracle.w8a16_gemm(x, w.q, w.s)
            assert np.array_equal(ref.astype(np.float32), want.astype(np.float32)), (case.id, e)
            _three_orders(p, x, deq.astype(np.float32))
    # every expert has its own codes and its own scales
    assert len({rp.w[e].q.tobytes() for e in range(rp.route.E)}) == rp.route.E and len({rp.w[e].s.tobytes() for e in range(rp.route.E)}) == rp.route.E


def _analyse(oracle, dc):
    if dc.id in _stats:
        return _stats[dc.id]
    rp = mc.Routed(dc.case, mc.decode_routing())
    _check_routed(oracle, rp)
    ref = rp.reference()
    assert np.all(ref[rp.route.used:] == mc.POISON) and not np.any(ref[:rp.route.used] == mc.POISON)
    stats = {}
    for name, (y, rows) in mc.decode_mutants(rp, dc).items():
        stats[name] = (ec.differs(y[rows], ref[rows]), mc.tier_a_accepts(rp, y, ref))
    _stats[dc.id] = stats
    return stats


def test_routing_table_is_the_one_the_cases_are_listed_for():
    r = mc.decode_routing()
    assert (r.E, r.k, r.T, r.S) == (8, 2, 43, 86) and tuple(r.counts) == mc.COUNTS
    assert sorted(r.idx.ravel().tolist()).count(8) == 1 and (r.idx == -1).sum() == 1
    assert r.offsets[r.E] == r.used == 84 < r.S
    assert r.active.tolist() == [1, 2, 3, 4, 5, 7, -1, -1]
    # the two slots of most tokens go to different experts: x[sorted_slot[p]] is then not x[sorted_slot[p] / k]
    assert (r.idx[:, 0] != r.idx[:, 1]).sum() > r.T * 2 // 3 and (r.idx[:, 0] == r.idx[:, 1]).any()
    for e in r.live():
        assert (r.slots(e) // r.k != r.slots(e) % r.T).any()
    assert np.array_equal(np.sort(r.sorted_slot[:r.used]), np.flatnonzero((r.idx.ravel() >= 0) & (r.idx.ravel() < 8)))
    assert all(np.all(np.diff(r.slots(e)) > 0) and np.all(r.idx.ravel()[r.slots(e)] == e) for e in r.live())       # a stable sort
    assert np.array_equal(r.position[r.sorted_slot[:r.used]], np.arange(r.used))


def test_every_k_selects_the_plan_and_the_tiles_it_is_listed_for():
    assert {(d.bits, d.K) for d in mc.DECODE_CASES} == set(mc.LISTED) and len(mc.DECODE_CASES) == 19
    for d in mc.DECODE_CASES:
        assert ((d.waves, d.depth), (d.tiles[0], d.tiles[-1])) == mc.LISTED[(d.bits, d.K)], d.id
        assert sum(d.tiles) == d.K // mc.tile_k(d.bits) and min(d.tiles) >= d.depth, d.id
    # the edges of the plan rule: the last K of a form and the first of the next
    for bits, edges in ((8, (7, 8, 15, 16)), (4, (1, 2, 3, 4, 63, 64))):
        assert {e * mc.tile_k(bits) for e in edges} <= set(mc.DECODE_K[bits])
    assert [mc.plan(8, 64 * t) for t in (7, 8, 15, 16)] == [(1, 1), (4, 2), (4, 2), (8, 2)]
    assert [mc.plan(4, 128 * t) for t in (1, 2, 3, 4, 63, 64)] == [(1, 1), (2, 1), (2, 1), (4, 1), (4, 1), (8, 2)]


def test_the_table_shows_every_feature_of_the_k_loop_each_instantiation_can_show():
    by = {}
    for d in mc.DECODE_CASES:
        by.setdefault((d.bits, d.waves, d.depth), set()).update(mc.features(d.bits, d.K))
    assert set(by) == {(8, 1, 1), (8, 4, 2), (8, 8, 2), (4, 1, 1), (4, 2, 1), (4, 4, 1), (4, 8, 2)}
    for (bits, waves, depth), seen in by.items():
        assert seen == mc.reachable(bits, waves, depth), (bits, waves, depth, seen)
        if depth == 2:
            assert {("r", 0), ("r", 1), ("unequal",), ("steady", True)} <= seen
        if waves > 1:
            assert ("unequal",) in seen
    # the steady loop not running: everywhere but on int4's 8 x 2 (64 tiles are 8 per wave) -- and running everywhere but on int4's
    # 1 x 1 (one K, one tile)
    assert {k for k, seen in by.items() if ("steady", False) not in seen} == {(4, 8, 2)}
    assert {k for k, seen in by.items() if ("steady", True) not in seen} == {(4, 1, 1)}


@pytest.mark.parametrize("dc", mc.DECODE_CASES, ids=lambda d: d.id)
def test_decode_inputs_meet_the_condition_and_every_mutant_shows(oracle, dc):
    stats = _analyse(oracle, dc)
    want = {"lost_first_k", "lost_last_k", "doubled_k", "lost_quietest_k", "doubled_quietest_k", "x_shifted_by_one_k", "last_tile_of_last_wave_lost",
            "last_tile_of_last_wave_doubled", "tail_tile_of_wave_0_lost", "weight_of_next_expert", "scales_of_next_expert", "x_row_of_the_slot",
            "clamped_row_stored_one_past"}
    assert want <= set(stats) and ("fp16_wave_partials" in stats) == (dc.waves > 1)
    for name, (share, _) in stats.items():
        assert share >= mc.MUTANT_FLOOR, (dc.id, name, share)


def test_which_mutants_tier_a_accepts(oracle):
    accepted = {}
    for dc in mc.DECODE_CASES:
        for name, (_, ok) in _analyse(oracle, dc).items():
            accepted.setdefault(name, [])
            if ok:
                accepted[name].append(dc.id)
    for name in sorted(accepted):
        print("%-34s tier A accepts it on %2d of %d cases  %s" % (name, len(accepted[name]), len(mc.DECODE_CASES), " ".join(i[11:] for i in accepted[name][:8])))
    # as seen here: ONE lost or doubled product (the quietest) and every early rounding pass tier A somewhere ...
    for name in ("lost_quietest_k_of_the_1_row_expert", "doubled_quietest_k_of_the_1_row_expert", "fp16_partials_of_2_slices", "fp16_partials_of_4_slices", "fp16_accumulator_every_64_k",
                 "fp16_wave_partials"):
        assert accepted[name], name
    # ... a whole k tile of one wave, another expert's weight or scales, the wrong row of x and a row stored one past never do
    for name in ("last_tile_of_last_wave_lost", "last_tile_of_last_wave_doubled", "tail_tile_of_wave_0_lost", "weight_of_next_expert", "scales_of_next_expert",
                 "x_row_of_the_slot", "clamped_row_stored_one_past", "x_shifted_by_one_k", "last_vector_shifted_by_one_k", "lost_quietest_k", "doubled_quietest_k"):
        assert not accepted[name], (name, accepted[name])


@pytest.mark.parametrize("case", mc.GRAD_CASES, ids=lambda c: c.id)
def test_gradient_inputs_meet_the_condition(oracle, case):
    assert case.K % 128 == (64 if case.bits == 8 else 0) and case.N % 64 == 16
    _check_routed(oracle, mc.Routed(case, mc.decode_routing()))


@pytest.mark.parametrize("case", mc.TILED_CASES, ids=lambda c: c.id)
def test_tiled_inputs_meet_the_condition(oracle, case):
    ids = np.array([0] * 127 + [2] * 128 + [3] * 129 + [5])[np.random.default_rng(case.K).permutation(385)].reshape(385, 1)
    rp = mc.Routed(case, mc.straddle_routing(ids))
    _check_routed(oracle, rp)
    # the ring minimum and the layout; one k tile less is K = 256 for either width: the first K the kernels refuse
    assert case.K // 64 >= 5 and (case.bits == 8 or (case.K % 128 == 0 and case.K >= 384)) and min(mc.TILED_K[case.bits]) - mc.tile_k(case.bits) == 256


_combine = {}


def _analyse_combine(c):
    if c.id not in _combine:
        p = mc.Combine(c)
        pr = p.products()
        # the condition, from the data: every product an integer of quanta, the sum of magnitudes below 2^24 (2^18 in fact)
        assert np.abs(p.i).max() <= 2047 and p.m.min() >= 0 and p.m.max() <= 16
        assert p.bound() < 2 ** 18 < mc.LIMIT, c.id
        want = p.reference()
        exact = (pr.sum(1) * p.quantum).astype(np.float32)
        assert np.array_equal(exact.astype(np.float64), pr.sum(1) * p.quantum)
        # fp32 products (each exact) added in three slot orders hold the exact sum
        pos = p.position.reshape(c.T, c.k)
        yv = np.where(p.live[:, :, None], np.nan_to_num(p.y[np.maximum(pos, 0)].astype(np.float32)), np.float32(0))
        terms = yv * p.w.astype(np.float32)[:, :, None]
        assert terms.dtype == np.float32
        fwd, rev = np.zeros((c.T, c.H), np.float32), np.zeros((c.T, c.H), np.float32)
        for j in range(c.k):
            fwd, rev = fwd + terms[:, j], rev + terms[:, c.k - 1 - j]
        pair = terms[:, 0::2].sum(1, dtype=np.float32) + (terms[:, 1::2].sum(1, dtype=np.float32) if c.k > 1 else 0)
        for name, y in (("forward", fwd), ("reversed", rev), ("pairs", pair)):
            assert np.array_equal(y.astype(np.float32), exact), (c.id, name)
        # the edges the case is there for
        named = np.zeros(len(p.y), bool)
        named[p.position[p.position >= 0]] = True
        assert np.isnan(p.y[~named]).all() and (~named).sum() >= mc.SPARE and np.isfinite(p.y[named]).all() and np.isfinite(want).all()
        if c.T > 1:
            assert not p.live[2].any() and not want[2].any() and ((p.position == -1).sum() == c.k + (c.k > 1))
        stats = {}
        for name, y in p.mutants().items():
            t = p.touched(name)
            stats[name] = (ec.differs(y[t], want[t]), bool(ac.tier_a(y, want).all()))
        _combine[c.id] = stats
    return _combine[c.id]


@pytest.mark.parametrize("c", mc.COMBINE_CASES, ids=lambda c: c.id)
def test_combine_inputs_meet_the_condition_and_every_mutant_shows(c):
    stats = _analyse_combine(c)
    assert set(stats) == ({"dropped_slot", "weight_of_next_slot", "products_rounded_to_fp16", "fp16_accumulator"} if c.k > 1 else {"dropped_slot"})
    for name, (share, _) in stats.items():
        assert share >= mc.MUTANT_FLOOR, (c.id, name, share)


def test_combine_cases_and_what_tier_a_makes_of_the_mutants():
    cs = mc.COMBINE_CASES
    assert len(cs) == 48 and {c.T for c in cs} == {1, 5} and {c.k for c in cs} == {1, 2, 8} and {c.H for c in cs} == {8, 2040, 2048, 2056}
    assert {c.wdtype for c in cs} == {"f32", "f16"}
    accepted = {}
    for c in cs:
        for name, (_, ok) in _analyse_combine(c).items():
            accepted.setdefault(name, [])
            if ok:
                accepted[name].append(c.id)
    for name in sorted(accepted):
        print("%-28s tier A accepts it on %2d of %d cases" % (name, len(accepted[name]), len(cs)))
    assert accepted["products_rounded_to_fp16"] and accepted["fp16_accumulator"]
    assert not accepted["dropped_slot"] and not accepted["weight_of_next_slot"]


def test_the_failure_report_names_the_expert_the_row_group_and_the_plan(oracle):
    """The GPU test's message on a result whose 33-row expert lost the last k tile of the last wave in its third 16-row group and the
    middle 16-column tile row."""
    from test_gpu_moe_exact import _explain
    dc = next(d for d in mc.DECODE_CASES if d.id == "moe-decode-i8-k1984")
    rp = mc.Routed(dc.case, mc.decode_routing())
    want, (bad, _) = rp.reference(), mc.decode_mutants(rp, dc)["last_tile_of_last_wave_lost"]
    got = want.copy()
    row = rp.route.offsets[5] + 32
    got[row, 16:32] = bad[row, 16:32]
    text = _explain(dc.id, rp, got, want, "%d x %d, k tiles per wave %s" % (dc.waves, dc.depth, dc.tiles))
    assert "experts [5]" in text and "16-row groups (expert, group) [(5, 2)]" in text and "16-column tile rows [1] (of 3)" in text, text
    assert "8 x 2" in text and "(4, 4, 4, 4, 4, 4, 4, 3)" in text and "quanta" in text and "first at row" in text, text
