"""window_cases.py pinned on the CPU: the windowed reference, the counts, the oldest-wins staircase and the census figures of the
cases test_gpu_window_attn.py and test_gpu_window_decode.py run, plus what the host side of the feature promises without a GPU
(the exported entries and their refusals, the promise context, the decoder's refused combinations)."""
import ctypes

import numpy as np
import pytest

import attn_cases as ac
import window_cases as wc

ENTRIES = ("eetq_prefill_attention_window_f16", "eetq_decode_attention_window_f16", "eetq_rope_decode_attention_window_f16")


def _brute(q, k, v, keys, koff, W, scale):
    """softmax over the window, one query at a time"""
    Bq, T, Hq, D = q.shape
    out = np.zeros((Bq, T, Hq, D))
    kk, vv = ac.expand_heads(k, Hq).astype(np.float64), ac.expand_heads(v, Hq).astype(np.float64)
    for t in range(T):
        p = t + koff
        lo, hi = max(0, p - W + 1), min(keys, p + 1)
        if hi <= lo:
            continue
        s = np.einsum("bhd,bhsd->bhs", q[:, t].astype(np.float64), kk[:, :, lo:hi]) * scale
        w = np.exp(s - s.max(-1, keepdims=True))
        out[:, t] = np.einsum("bhs,bhsd->bhd", w, vv[:, :, lo:hi]) / w.sum(-1)[..., None]
    return out


def test_reference_and_counts():
    c = ac.prefill_random_case(2, 9, 4, 2, 23, 64, seed=3)
    koff = 23 - 9
    plain, plain_abs = ac.prefill_reference(c["q"], c["k"], c["v"], 23, koff, c["scale"])
    for W in (23, 24, 1000):     # W >= keys: the plain reference
        out, absmean = wc.window_reference(c["q"], c["k"], c["v"], 23, koff, W, c["scale"])
        assert np.array_equal(out, plain) and np.array_equal(absmean, plain_abs)
        assert np.array_equal(wc.window_counts(9, 23, koff, W), ac.prefill_counts(9, 23, koff))
    for W in (1, 2, 5, 16):
        out, _ = wc.window_reference(c["q"], c["k"], c["v"], 23, koff, W, c["scale"])
        assert np.allclose(out, _brute(c["q"], c["k"], c["v"], 23, koff, W, c["scale"]), rtol=1e-12, atol=1e-12)
        assert np.array_equal(wc.window_counts(9, 23, koff, W), np.minimum(W, np.arange(9) + koff + 1))
        assert np.array_equal(wc.window_allowed(9, 23, koff, W).sum(-1), wc.window_counts(9, 23, koff, W))
    # W = 1: the row itself
    out, _ = wc.window_reference(c["q"], c["k"], c["v"], 23, koff, 1, c["scale"])
    assert np.array_equal(out, ac.expand_heads(c["v"][:, :, koff:23], 4).transpose(0, 2, 1, 3).astype(np.float64))
    # keys short of the query rows: the first queries attend nothing
    assert list(wc.window_counts(4, 2, -2, 3)) == [0, 0, 1, 2]
    assert wc.decode_window_start(10, 4) == 6 and wc.decode_window_start(3, 4) == 0 and wc.decode_window_start(10, 4, 8) == 8


def test_winner_is_the_oldest_placed_row_inside_the_window():
    rows, ranks = np.array([3, 4, 9]), np.array([3, 2, 1])
    win = wc.window_winner(12, 0, 3, rows, ranks)
    #        t:  0   1   2  3  4  5  6   7   8  9  10 11
    assert list(win) == [-1, -1, -1, 3, 3, 3, 4, -1, -1, 9, 9, 9]
    assert list(wc.edge_queries(12, 0, 3, rows)) == [6]            # row 3 just outside, row 4 just inside
    assert list(wc.window_winner(4, 8, 100, rows, ranks)) == [3, 3, 3, 3]


@pytest.mark.parametrize("shape", sorted(wc.SHAPES))
@pytest.mark.parametrize("D", wc.DIMS)
def test_staircase_cases_meet_the_gap_and_reach_every_edge(shape, D):
    c = wc.staircase_case(shape, D, seed=11 + D)
    assert wc.staircase_gap(c) >= ac.GAP_MIN
    assert np.isfinite(c["k"][:, :, :c["keys"]].astype(np.float64)).all()
    T, keys, koff = c["T"], c["keys"], c["koff"]
    for W in wc.windows(keys):
        win = wc.window_winner(T, koff, W, c["placed"], c["ranks"])
        if W >= keys:
            continue
        edges = wc.edge_queries(T, koff, W, c["placed"])
        if W > 1:
            assert edges.size, (shape, W, "no query has a placed row just outside and one just inside its window")
            # at an edge the winner is the row just inside, and the row just outside outranks it: a leak would win
            assert all(win[t] == t + koff - W + 1 for t in edges)
    # a 64-key block boundary between the outside and the inside row, and a wave's 32-row boundary between two edge queries
    pairs = [(r, r + 1) for r in c["placed"] if r + 1 in set(c["placed"])]
    assert any((r + 1) % 64 == 0 for r, _ in pairs)
    ts = set()
    for W in wc.windows(keys):
        ts |= set(int(t) for t in wc.edge_queries(T, koff, W, c["placed"]))
    assert any(t % 32 == 31 and t + 1 in ts for t in ts)


@pytest.mark.parametrize("shape", sorted(wc.SHAPES))
@pytest.mark.parametrize("D", wc.DIMS)
def test_census_cases_show_a_dropped_and_a_doubled_row(shape, D):
    c = wc.census_case(shape, D, seed=5 + D)
    T, keys, koff = c["T"], c["keys"], c["koff"]
    for W in wc.windows(keys):
        drop, dbl = wc.window_census_shift_ulps(c["v"], T, keys, koff, W)
        assert drop >= 1.0, (shape, W, drop)
        assert (dbl is None) == (W == 1) and (dbl is None or dbl >= 1.0), (shape, W, dbl)
        mean = wc.window_census_mean(c["v"], T, keys, koff, W)
        ref, _ = wc.window_reference(c["q"], c["k"], c["v"], keys, koff, W, c["scale"])
        assert np.allclose(ac.expand_heads(mean.transpose(0, 2, 1, 3), wc.H).transpose(0, 2, 1, 3), ref, rtol=1e-12, atol=1e-12)


def test_decode_census_shows_a_dropped_and_a_doubled_row():
    """the one census case of test_gpu_window_decode.py: the last 65 of 200 rows"""
    v, _ = ac.census_values(3, 2, 200, 64, seed=9)
    drop, dbl = ac.census_shift_ulps(v[:, :, 135:200], 65)
    assert drop >= 1.0 and dbl >= 1.0


# ---- the host side ---------------------------------------------------------------------------------------------------------------

def test_entries_are_exported_and_refuse_a_window_below_one():
    from eetq_amd import _lib
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    st = (ctypes.c_long * 12)(*([64] * 12))
    for w in (0, -3):
        assert lib.eetq_prefill_attention_window_f16(p, p, p, p, None, 1, 2, 1, 4, 8, 64, None, 0, w, 1, 0.125, st, None) == -1
        assert b"window" in lib.eetq_last_error()
        assert lib.eetq_decode_attention_window_f16(p, p, p, None, p, p, 1, 2, 1, 8, 64, 1, 0.125, st, None, 0, None, w, None,
                                                    None) == -1
        assert b"window" in lib.eetq_last_error()
        assert lib.eetq_rope_decode_attention_window_f16(p, None, 0, p, p, p, p, 16, p, p, None, p, p, p, 1, 2, 1, 8, 64, 1, 0.125,
                                                         st, None, 0, None, w, None, None) == -1
        assert b"window" in lib.eetq_last_error()
    # the checks of the entries they extend still answer
    assert lib.eetq_prefill_attention_window_f16(p, p, p, p, None, 1, 2, 1, 4, 8, 96, None, 0, 4, 1, 0.125, st, None) == -3   # head_dim
    assert lib.eetq_prefill_attention_window_f16(p, None, p, p, None, 1, 2, 1, 4, 8, 64, None, 0, 4, 1, 0.125, st, None) == -1
    assert lib.eetq_decode_attention_window_f16(p, p, p, None, p, p, 1, 3, 2, 8, 64, 1, 0.125, st, None, 0, None, 4, None,
                                                None) == -1
    assert b"invalid attention shape" in lib.eetq_last_error()


def test_promise_context_and_its_refusals():
    from eetq_amd.modules import llama_modules as lm
    assert lm._window() is None
    with lm.sliding_window_static(6):
        assert lm._window() == 6
        with lm.sliding_window_static(9):
            assert lm._window() == 9
        assert lm._window() == 6
        with pytest.raises(ValueError, match="sliding_window_static"):
            with lm.padded_static_batch(object()):
                pass
        with pytest.raises(ValueError, match="sliding window"):
            with lm.appended_static_prefill(few_rows=True):
                pass
        with pytest.raises(ValueError, match="sliding window"):
            with lm.appended_static_prefill(int8_rows=True, few_rows_int8=True):
                pass
        with lm.appended_static_prefill(), lm.padded_static_batch(None):
            assert lm._window() == 6
    assert lm._window() is None
    for bad in (0, -1, True, 2.5, "4"):
        with pytest.raises(ValueError, match="window"):
            with lm.sliding_window_static(bad):
                pass
    with lm.padded_static_batch(object()):
        with pytest.raises(ValueError, match="padded_static_batch"):
            with lm.sliding_window_static(4):
                pass
    with lm.appended_static_prefill(few_rows=True):
        with pytest.raises(ValueError, match="few_rows"):
            with lm.sliding_window_static(4):
                pass
    with lm.sliding_window_static(None):
        assert lm._window() is None


def test_decoder_refuses_what_has_no_window():
    from eetq_amd.utils.graph_decoder import GraphDecoder
    chk = GraphDecoder._check_window
    assert chk(None, None, True, False, 16, 0) is None
    for bad in (0, -2, True, 1.5):
        with pytest.raises(ValueError, match="window must be"):
            chk(bad, None, True, False, 16, 0)
    with pytest.raises(ValueError, match="ragged"):
        chk(6, None, True, True, 16, 0)
    with pytest.raises(ValueError, match="kv_bits"):
        chk(6, None, True, False, 8, 0)
    with pytest.raises(ValueError, match="speculative"):
        chk(6, None, True, False, 16, 3)
    with pytest.raises(ValueError, match="fully accelerated"):
        chk(6, object(), True, False, 16, 0)
