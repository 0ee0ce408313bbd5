"""The attention modules' promises and the two route decisions, without a GPU.

The promise matrix nests every ordered pair of nine entries of the four context managers and checks which pairs are refused, what
the state reads inside, and that a refusal, an exit and an exception in the body all leave the state as it was.  The route tables
run ``_route_fp16`` and ``_route_int8`` over the full product of their inputs against a literal transcription of their ordered
rules, written out below without a call of the functions under test."""
import itertools
import threading

import pytest

import eetq_amd.modules.llama_modules as lm

FIELDS = ("fresh", "appended", "int8_rows", "few_rows", "few_rows_int8", "starts", "window")
DEFAULTS = dict(fresh=False, appended=False, int8_rows=False, few_rows=False, few_rows_int8=False, starts=None, window=None)
OBJ = object()


def _appended(**flags):
    return dict(dict(appended=True, fresh=False, int8_rows=False, few_rows=False, few_rows_int8=False), **flags)


# name -> (the manager's call, the fields it sets)
ENTRIES = {
    "fresh": (lambda: lm.fresh_static_prefill(), dict(fresh=True)),
    "appended()": (lambda: lm.appended_static_prefill(), _appended()),
    "appended(int8_rows)": (lambda: lm.appended_static_prefill(int8_rows=True), _appended(int8_rows=True)),
    "appended(few_rows)": (lambda: lm.appended_static_prefill(few_rows=True), _appended(few_rows=True)),
    "appended(int8_rows,few_rows_int8)": (lambda: lm.appended_static_prefill(int8_rows=True, few_rows_int8=True),
                                          _appended(int8_rows=True, few_rows_int8=True)),
    "padded(obj)": (lambda: lm.padded_static_batch(OBJ), dict(starts=OBJ)),
    "padded(None)": (lambda: lm.padded_static_batch(None), dict(starts=None)),
    "window(4)": (lambda: lm.sliding_window_static(4), dict(window=4)),
    "window(None)": (lambda: lm.sliding_window_static(None), dict(window=None)),
}
_PAIRS = [("appended(few_rows)", "padded(obj)"), ("appended(few_rows)", "window(4)"),
          ("appended(int8_rows,few_rows_int8)", "padded(obj)"), ("appended(int8_rows,few_rows_int8)", "window(4)"),
          ("padded(obj)", "window(4)")]
REFUSED = set(_PAIRS) | {(b, a) for a, b in _PAIRS}
NESTINGS = list(itertools.product(ENTRIES, ENTRIES))


def state():
    p = lm._prefill_promise
    return {f: getattr(p, f, DEFAULTS[f]) for f in FIELDS}


def test_the_matrix_has_nine_entries_and_ten_refusals():
    assert len(ENTRIES) == 9 and len(NESTINGS) == 81 and len(REFUSED) == 10 and REFUSED <= set(NESTINGS)


@pytest.mark.parametrize("outer,inner", NESTINGS, ids=["%s>%s" % n for n in NESTINGS])
def test_promise_matrix(outer, inner):
    assert state() == DEFAULTS
    (enter_a, set_a), (enter_b, set_b) = ENTRIES[outer], ENTRIES[inner]
    with enter_a():
        s_a = dict(DEFAULTS, **set_a)
        assert state() == s_a
        if (outer, inner) in REFUSED:
            with pytest.raises(ValueError):
                with enter_b():
                    pytest.fail("a refused promise was entered")
        else:
            with enter_b():
                assert state() == dict(s_a, **set_b)     # the entered manager's fields over the outer state
            assert state() == s_a
            with pytest.raises(KeyError):
                with enter_b():
                    raise KeyError("x")
        assert state() == s_a
    assert state() == DEFAULTS
    with pytest.raises(KeyError):
        with enter_a():
            raise KeyError("x")
    assert state() == DEFAULTS


@pytest.mark.parametrize("outer,inner", sorted(REFUSED), ids=["%s>%s" % n for n in sorted(REFUSED)])
def test_a_refusal_names_the_entered_manager_and_both_promises(outer, inner):
    manager = {"f": "fresh_static_prefill", "a": "appended_static_prefill", "p": "padded_static_batch", "w": "sliding_window_static"}
    with ENTRIES[outer][0]():
        with pytest.raises(ValueError) as err:
            with ENTRIES[inner][0]():
                pass
    text = str(err.value)
    assert text.startswith(manager[inner[0]] + ":")
    for name in (outer, inner):
        if name.startswith("appended"):
            assert ("few_rows_int8" if "few_rows_int8" in name else "few_rows") in text
        else:
            assert manager[name[0]] in text
    reasons = ("one shared first key only", "has no sliding window", "reads fp16 cache rows only")
    assert sum(r in text for r in reasons) == 1


def test_another_thread_sees_nothing_promised():
    seen = []
    with lm.appended_static_prefill(int8_rows=True, few_rows_int8=True), lm.fresh_static_prefill():
        t = threading.Thread(target=lambda: seen.append(state()))
        t.start()
        t.join()
        assert state() == dict(DEFAULTS, fresh=True, appended=True, int8_rows=True, few_rows_int8=True)
    with lm.padded_static_batch(OBJ):
        t = threading.Thread(target=lambda: seen.append(state()))
        t.start()
        t.join()
    assert seen == [DEFAULTS, DEFAULTS] and state() == DEFAULTS


OWN_ARGUMENTS = [
    ("few_rows_int8 without int8_rows", lambda: lm.appended_static_prefill(few_rows_int8=True), "needs int8_rows=True"),
    ("few_rows with int8_rows", lambda: lm.appended_static_prefill(int8_rows=True, few_rows=True), "fp16 cache rows only"),
    ("window=0", lambda: lm.sliding_window_static(0), "window must be an integer"),
]


@pytest.mark.parametrize("outer", [None] + list(ENTRIES))
@pytest.mark.parametrize("what,enter,match", OWN_ARGUMENTS, ids=[o[0] for o in OWN_ARGUMENTS])
def test_own_argument_errors_come_first(outer, what, enter, match):
    # ("window(4)", "few_rows with int8_rows") is the one case that differs from the code before the conflict table: there
    # appended_static_prefill looked at the window before its own two row flags and reported the window conflict
    with (ENTRIES[outer][0]() if outer else lm.padded_static_batch(None)):
        before = state()
        with pytest.raises(ValueError, match=match):
            with enter():
                pass
        assert state() == before
    assert state() == DEFAULTS


def test_every_promise_is_exported():
    for name in ("fresh_static_prefill", "appended_static_prefill", "padded_static_batch", "sliding_window_static"):
        assert name in lm.__all__


# ---- the route tables ------------------------------------------------------------------------------------------------------------

class Promise:
    def __init__(self, **fields):
        self.__dict__.update(DEFAULTS, **fields)


MODES = {"none": (False, False), "fresh": (True, False), "appended": (False, True), "both": (True, True)}


def expected_fp16(fresh, appended, few_rows, starts, window, cached, T, weights, mfma_ok, rows_ok):
    """the ordered rules of the fp16 static-cache path: (operator, fresh form, extra keywords) or (exception type, a word of its text)"""
    mode = "fresh" if fresh else "appended" if appended else None
    if window is not None:                                                                      # 1
        if starts is None and cached and T > 1 and not weights and mfma_ok and mode is not None and not few_rows:
            return ("prompt", mode == "fresh", {"window": window})
        return (ValueError, "sliding_window_static needs")
    if starts is not None:                                                                      # 2
        if cached and T > 1 and not weights and mfma_ok and mode is not None:
            return ("prompt", mode == "fresh", {"kv_start": starts})
        return (ValueError, "padded_static_batch needs")
    if cached:                                                                                  # 3
        if mode == "appended" and few_rows and 2 <= T <= 16 and rows_ok and not weights:
            return ("rows", False, {})
        if mode == "appended" and T > 1 and not weights and mfma_ok:
            return ("prompt", False, {})
        if mode == "fresh" and T > 1 and not weights:
            return ("prompt", True, {}) if mfma_ok else ("sdpa", True, {})
        return ("stock", False, {})
    return ("stock", False, {})                                                               # 4


FP16_PRODUCT = list(itertools.product(MODES, (False, True), (None, OBJ), (None, 4), (False, True), (1, 2, 16, 17), (False, True),
                                      (False, True), (False, True)))


def _outcome(fn, *args):
    try:
        return tuple(fn(*args))
    except (ValueError, NotImplementedError) as e:
        return type(e), str(e)


def test_fp16_route_table():
    assert len(FP16_PRODUCT) == 4 * 2 * 2 * 2 * 2 * 4 * 2 * 2 * 2
    seen = set()
    for mode, few_rows, starts, window, cached, T, weights, mfma_ok, rows_ok in FP16_PRODUCT:
        fresh, appended = MODES[mode]
        want = expected_fp16(fresh, appended, few_rows, starts, window, cached, T, weights, mfma_ok, rows_ok)
        p = Promise(fresh=fresh, appended=appended, few_rows=few_rows, starts=starts, window=window)
        got = _outcome(lm._route_fp16, p, cached, T, weights, mfma_ok, rows_ok)
        case = (mode, few_rows, starts, window, cached, T, weights, mfma_ok, rows_ok)
        if isinstance(want[0], type):
            assert got[0] is want[0] and want[1] in got[1], (case, got)
        else:
            assert got == want, (case, got)
        seen.add((want[0], ) + tuple(want[2]) if isinstance(want[0], str) else want)
    # every route and both refusals occur in the product
    assert seen == {("prompt", "window"), ("prompt", "kv_start"), ("prompt",), ("rows",), ("sdpa",), ("stock",),
                    (ValueError, "sliding_window_static needs"), (ValueError, "padded_static_batch needs")}


ROWS = 64


def expected_int8(fresh, appended, int8_rows, few_rows_int8, starts, window, T, supported, table_ok, prompt8_ok, rows8_ok, mfma_ok):
    """the int8 cache's ordered rules: a route name or (exception type, a word of its text)"""
    if window is not None:                                                                      # 1
        return (ValueError, "sliding_window_static needs an fp16 static cache")
    if starts is not None:                                                                      # 2
        return (ValueError, "padded_static_batch (a left-padded batch) needs an fp16 static cache")
    if not supported:                                                                           # 3
        return (NotImplementedError, "an int8 KV cache needs float16 on the GPU")
    if not table_ok:
        return (NotImplementedError, "the rotation to cover the whole head")
    if T == 1:                                                                                  # 4
        return "decode"
    if appended and not fresh and int8_rows:                                                    # 5
        if T > ROWS:
            return (ValueError, "longer than the cache")
        if not prompt8_ok:
            return (NotImplementedError, "int8 K and V")
        if few_rows_int8 and 2 <= T <= 16:
            if not rows8_ok:
                return (NotImplementedError, "ops.decode_attention_rows_i8kv")
            return "rows_i8"
        return "prompt_i8"
    if not fresh or appended:                                                                   # 6: fresh inside appended too
        return (NotImplementedError, "promised fresh")
    if T > ROWS:                                                                                # 7
        return (ValueError, "longer than the cache")
    return "prompt" if mfma_ok else "sdpa"


INT8_PRODUCT = list(itertools.product(MODES, (False, True), (False, True), (None, OBJ), (None, 4), (1, 2, 16, 17, ROWS + 1),
                                      (False, True), (False, True), (False, True), (False, True), (False, True)))


def test_int8_route_table():
    assert len(INT8_PRODUCT) == 4 * 2 * 2 * 2 * 2 * 5 * 2 ** 5
    seen = set()
    for mode, int8_rows, few8, starts, window, T, supported, table_ok, prompt8_ok, rows8_ok, mfma_ok in INT8_PRODUCT:
        fresh, appended = MODES[mode]
        want = expected_int8(fresh, appended, int8_rows, few8, starts, window, T, supported, table_ok, prompt8_ok, rows8_ok, mfma_ok)
        p = Promise(fresh=fresh, appended=appended, int8_rows=int8_rows, few_rows_int8=few8, starts=starts, window=window)
        try:
            got = lm._route_int8(p, T, ROWS, supported, table_ok, prompt8_ok, rows8_ok, mfma_ok)
        except (ValueError, NotImplementedError) as e:
            got = (type(e), str(e))
        case = (mode, int8_rows, few8, starts, window, T, supported, table_ok, prompt8_ok, rows8_ok, mfma_ok)
        if isinstance(want, tuple):
            assert isinstance(got, tuple) and got[0] is want[0] and want[1] in got[1], (case, got)
        else:
            assert got == want, (case, got)
        seen.add(want if isinstance(want, str) else want[1])
    assert {"decode", "rows_i8", "prompt_i8", "prompt", "sdpa", "promised fresh", "longer than the cache"} <= seen
    # the quirk, kept on purpose: fresh_static_prefill entered inside appended_static_prefill is "fresh" on an fp16 cache and
    # a refusal on an int8 cache, with or without int8_rows
    for int8_rows in (False, True):
        p = Promise(fresh=True, appended=True, int8_rows=int8_rows)
        with pytest.raises(NotImplementedError, match="promised fresh"):
            lm._route_int8(p, 5, ROWS, True, True, True, True, True)
        assert tuple(lm._route_fp16(p, True, 5, False, True, True)) == ("prompt", True, {})
