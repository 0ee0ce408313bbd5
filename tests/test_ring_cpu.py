"""The ring cache's host side, without a GPU: ``ring_rows`` against the capacity rule, the ring promise of
``sliding_window_static``, the route it gives, ``GraphDecoder``'s own-argument checks, and a numpy restatement of the addressing
-- logical row -> physical row, the rows a prompt launch reads, the rows its cache write replaces -- that shows the rule keeps a
launch from reading what it has just overwritten, and that 64 rows fewer do not."""
import types

import numpy as np
import pytest

import eetq_amd.modules.llama_modules as lm
from eetq_amd.utils.graph_decoder import GraphDecoder
from eetq_amd.utils.kv_cache import ring_rows

GRID = [(W, T) for W in (1, 2, 5, 63, 64, 65, 100, 1000, 1024, 4096) for T in (1, 2, 4, 63, 64, 65, 128, 130, 512)]


@pytest.mark.parametrize("W,T", GRID)
def test_ring_rows_is_the_least_multiple_of_64_the_rule_admits(W, T):
    R = ring_rows(W, T)
    assert R % 64 == 0 and R >= W + T + 62 and R - 64 < W + T + 62
    assert R >= W, "a decode step's live rows fit as well"


def test_ring_rows_refuses_what_is_no_row_count():
    for bad in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError, match="window must be"):
            ring_rows(bad, 4)
        with pytest.raises(ValueError, match="chunk must be"):
            ring_rows(4, bad)


# ---- the promise ----
def _state():
    p = lm._prefill_promise
    return {f: getattr(p, f) for f in lm._PROMISE_FIELDS}


def test_the_promise_record_has_a_ring_field():
    assert "ring" in lm._PROMISE_FIELDS and _state()["ring"] is False and _state()["window"] is None


def test_ring_promise_sets_and_restores():
    before = _state()
    with lm.sliding_window_static(6, ring=True):
        assert _state() == dict(before, window=6, ring=True)
        with lm.sliding_window_static(4):            # an inner plain window promises no ring
            assert _state() == dict(before, window=4, ring=False)
        assert _state() == dict(before, window=6, ring=True)
        with lm.appended_static_prefill():
            assert _state() == dict(before, window=6, ring=True, appended=True)
    assert _state() == before
    with pytest.raises(KeyError):
        with lm.sliding_window_static(6, ring=True):
            raise KeyError("x")
    assert _state() == before


@pytest.mark.parametrize("outer", (None, "fresh", "appended", "window"))
def test_ring_without_a_window_is_refused_and_leaves_the_state(outer):
    enter = {None: lambda: lm.padded_static_batch(None), "fresh": lm.fresh_static_prefill, "appended": lm.appended_static_prefill,
             "window": lambda: lm.sliding_window_static(3, ring=True)}[outer]
    with enter():
        before = _state()
        with pytest.raises(ValueError, match="sliding_window_static: ring=True needs a window"):
            with lm.sliding_window_static(None, ring=True):
                pytest.fail("a refused promise was entered")
        with pytest.raises(ValueError, match="window must be an integer"):
            with lm.sliding_window_static(0, ring=True):
                pytest.fail("a refused promise was entered")
        assert _state() == before
    assert _state()["ring"] is False and _state()["window"] is None


def test_windows_refusals_cover_the_ring():
    """ring lives only with window: int8 rows, few_rows and padded_static_batch are refused by the window's own conflicts"""
    with lm.sliding_window_static(6, ring=True):
        for enter in (lambda: lm.appended_static_prefill(few_rows=True), lambda: lm.padded_static_batch(object()),
                      lambda: lm.appended_static_prefill(int8_rows=True, few_rows_int8=True)):
            with pytest.raises(ValueError):
                with enter():
                    pytest.fail("a refused promise was entered")
    p = types.SimpleNamespace(fresh=False, appended=True, int8_rows=True, few_rows=False, few_rows_int8=False, starts=None, window=6,
                              ring=True)
    with pytest.raises(ValueError, match="int8 kernels have no sliding window"):
        lm._route_int8(p, 4, 128, True, True, True, True, True)


@pytest.mark.parametrize("rows,W,T,ok", [(128, 6, 4, True), (128, 6, 60, True), (128, 6, 61, False), (64, 6, 4, False),
                                         (100, 6, 4, False), (ring_rows(4096, 512), 4096, 512, True),
                                         (ring_rows(4096, 512), 4096, 513 + 63, False)])
def test_a_prompt_call_longer_than_the_chunk_is_refused(rows, W, T, ok):
    if ok:
        lm._ring_prompt_check(rows, W, T)
    else:
        with pytest.raises(ValueError, match="exceeds the chunk of this ring cache"):
            lm._ring_prompt_check(rows, W, T)


# ---- the route ----
def _promise(**kw):
    base = dict(fresh=False, appended=False, int8_rows=False, few_rows=False, few_rows_int8=False, starts=None, window=None)
    return types.SimpleNamespace(**dict(base, **kw))


@pytest.mark.parametrize("fresh", (True, False))
def test_route_under_the_ring_promise(fresh):
    kind = dict(fresh=True) if fresh else dict(appended=True)
    ring = lm._route_fp16(_promise(window=6, ring=True, **kind), True, 4, False, True, True)
    assert ring.op == "prompt" and ring.fresh is fresh and ring.extra == {"window": 6, "ring": True}
    for p in (_promise(window=6, ring=False, **kind), _promise(window=6, **kind)):     # the second: a record without the field
        plain = lm._route_fp16(p, True, 4, False, True, True)
        assert plain.op == "prompt" and plain.extra == {"window": 6}
    assert lm._route_fp16(_promise(**kind), True, 4, False, True, True).extra == {}
    with pytest.raises(ValueError, match="sliding_window_static needs the MFMA prompt kernel"):
        lm._route_fp16(_promise(window=6, ring=True, **kind), True, 4, False, False, True)


# ---- GraphDecoder's own arguments ----
def test_rolling_own_argument_checks():
    check = GraphDecoder._check_rolling
    assert check(False, 512, None, False, 16, 0) == (False, None)
    assert check(True, 4, 6, False, 16, 0) == (True, 4)
    for args, match in (((True, 4, None, False, 16, 0), "rolling=True needs window"), ((True, 4, 6, True, 16, 0), "ragged"),
                        ((True, 4, 6, False, 8, 0), "kv_bits"), ((True, 4, 6, False, 16, 3), "speculative"),
                        ((True, 0, 6, False, 16, 0), "rolling_chunk"), ((True, True, 6, False, 16, 0), "rolling_chunk")):
        with pytest.raises(ValueError, match=match):
            check(*args)


# ---- the addressing, restated ----
def launch_rows(koff, T, W):
    """logical rows one prompt launch READS (whole 64-row key blocks from the lowest needed one to the last query's) and the rows
    its cache write has just WRITTEN"""
    lowest = 64 * (max(0, koff - W + 1) // 64)
    highest_block_end = 64 * ((koff + T - 1) // 64) + 64
    return np.arange(lowest, highest_block_end), np.arange(koff, koff + T)


def overwritten_reads(koff, T, W, R):
    """logical rows below koff that the launch reads although the write has replaced them: row r is lost once a written row w > r
    shares its physical row, w = r (mod R).  (Rows at and above koff + T that a read block covers are never valid: masked.)"""
    read, written = launch_rows(koff, T, W)
    phys_written = set((written % R).tolist())
    return [int(r) for r in read if r < koff and int(r % R) in phys_written]


@pytest.mark.parametrize("W,T", [(1, 5), (7, 64), (64, 65), (100, 130), (6, 4), (1024, 512), (4096, 512), (63, 1), (65, 63)])
def test_the_rule_keeps_a_launch_off_its_own_rows(W, T):
    R = ring_rows(W, T)
    koffs = sorted(set([0, 1, W - 1, W, W + 61, W + 62, W + 63, R - T, R - 1, R, R + 1, 2 * R - T // 2, 2 * R + 61, 5 * R + 17]
                       + list(range(3 * R, 3 * R + 64, 7))))
    for koff in (k for k in koffs if k >= 0):
        assert overwritten_reads(koff, T, W, R) == [], (W, T, R, koff)
        read, written = launch_rows(koff, T, W)
        # every block the launch reads lies inside the ring as one piece: 64 | R
        assert all((b % R) + 64 <= R for b in read[::64])
        # attended rows are all present: the youngest R rows are the ring's content
        assert koff + T - 1 - max(0, koff - W + 1) < R
    # 64 rows fewer can lose a row: some koff makes the launch read a block its own rows have replaced
    small = R - 64
    if small >= 64:
        assert small < W + T + 62
        assert any(overwritten_reads(koff, T, W, small) for koff in range(small, 3 * small)), (W, T, small)


def test_decode_rows_of_a_step():
    """a decode step at logical length n reads rows max(0, n - W) .. n - 1 and writes n - 1: with R >= W they are distinct physical
    rows, and with R = W - 1 the oldest attended row is the one just replaced"""
    for W in (1, 5, 16, 33, 300):
        for R in (W, W + 1, 64 * (-(-W // 64))):
            for n in (1, W - 1, W, W + 1, R - 1, R, R + 1, 2 * R, 3 * R + 4):
                if n < 1:
                    continue
                rows = np.arange(max(0, n - W), n)
                assert len(set((rows % R).tolist())) == len(rows), (W, R, n)
        if W > 1:
            n = 3 * W
            rows = np.arange(n - W, n)
            assert len(set((rows % (W - 1)).tolist())) < len(rows)
