"""Speculative greedy decoding (eetq_spec_ngram_draft_i64, eetq_spec_accept_f16), everything that needs no GPU: the entries'
surface in the header, the library and both bindings, every argument refusal, and the NumPy references (tests/spec_ref.py) on
hand-written cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spec_ref as ref
from conftest import ROOT

DRAFT, ACCEPT = "eetq_spec_ngram_draft_i64", "eetq_spec_accept_f16"


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_entry_surface(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr and lib.eetq_abi_version() == 7
    history = hdr[hdr.index("Revision history"):hdr.index("#define EETQ_AMD_ABI_VERSION")]
    for name, nargs in ((DRAFT, 10), (ACCEPT, 21)):
        assert re.search(r"\bint\s+%s\s*\(" % name, code)
        assert name in history                                  # listed among the entries added within revision 7
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is ctypes.c_int
    assert re.search(r"SRCS\s*:=.*\bspec\.hip", open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read())


def test_bindings():
    from eetq_amd import ops, ops_ctypes
    for name in ("ngram_draft", "spec_accept"):
        assert name in ops.__all__ and callable(getattr(ops, name))
        assert name in ops_ctypes.__all__ and callable(getattr(ops_ctypes, name))
    z = torch.zeros(1, dtype=torch.int64)
    for mod in (ops, ops_ctypes):                               # the checks run before any device work
        with pytest.raises(RuntimeError, match="int64 CUDA"):
            mod.ngram_draft(torch.zeros(1, 8, dtype=torch.int64), z, torch.zeros(1, 4, dtype=torch.int64), 3)
        with pytest.raises(RuntimeError, match="float16 CUDA"):
            mod.spec_accept(torch.zeros(1, 5, 8), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int64), z, z, z, z,
                            torch.zeros(1, 8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))


def _buffer():
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 8 == 0
    return buf, p


def test_draft_refusals_without_a_device(lib):
    buf, p = _buffer()
    good = dict(hist=p, hist_stride=64, cols=64, batch=2, position=p, max_ngram=3, k=4, draft=p, draft_stride=4, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.eetq_spec_ngram_draft_i64(*[a[key] for key in good])

    for arg in ("hist", "position", "draft"):
        assert call(**{arg: None}) == -1
        assert arg.encode() in lib.eetq_last_error(), (arg, lib.eetq_last_error())
        assert call(**{arg: ctypes.c_void_p(p.value + 4)}) == -1
        assert b"aligned" in lib.eetq_last_error(), (arg, lib.eetq_last_error())
    for arg, bad, word in (("max_ngram", 0, b"max_ngram"), ("max_ngram", 9, b"max_ngram"), ("k", 0, b"k must"), ("k", 16, b"k must"),
                           ("batch", 0, b"batch"), ("batch", -2, b"batch"), ("cols", 0, b"cols"), ("hist_stride", 63, b"stride"),
                           ("draft_stride", 3, b"stride")):
        assert call(**{arg: bad}) == -1
        assert word in lib.eetq_last_error(), (arg, bad, lib.eetq_last_error())
    del buf


def test_accept_refusals_without_a_device(lib):
    buf, p = _buffer()
    good = dict(logits=p, stride_b=5 * 64, stride_t=64, vocab=64, batch=2, k=4, draft=p, draft_stride=4, out_tokens=p, out_stride=8,
                out_cols=8, column=p, position=p, limit=p, next_token=p, next_stride=1, hist=p, hist_stride=16, hist_cols=16,
                stats=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.eetq_spec_accept_f16(*[a[key] for key in good])

    for arg in ("logits", "draft", "out_tokens", "column", "position", "limit", "next_token", "hist", "stats"):
        assert call(**{arg: None}) == -1
        assert arg.encode() in lib.eetq_last_error(), (arg, lib.eetq_last_error())
        if arg != "logits":
            assert call(**{arg: ctypes.c_void_p(p.value + 4)}) == -1
            assert b"aligned" in lib.eetq_last_error(), (arg, lib.eetq_last_error())
    assert call(logits=ctypes.c_void_p(p.value + 1)) == -1 and b"aligned" in lib.eetq_last_error()
    for arg, bad, word in (("k", 0, b"k must"), ("k", 16, b"k must"), ("vocab", 0, b"vocab"), ("vocab", -5, b"vocab"),
                           ("batch", 0, b"batch"), ("batch", -1, b"batch"), ("stride_t", 63, b"stride"), ("stride_b", 63, b"stride"),
                           ("draft_stride", 3, b"stride"), ("out_cols", 0, b"out_cols"), ("out_stride", 7, b"out_stride"),
                           ("hist_cols", 0, b"cols"), ("hist_stride", 15, b"stride"), ("next_stride", 0, b"next_token")):
        assert call(**{arg: bad}) == -1
        assert word in lib.eetq_last_error(), (arg, bad, lib.eetq_last_error())
    del buf


def test_draft_reference_on_hand_written_cases():
    d = lambda hist, N, k, pos=None: ref.ngram_draft_ref([hist], len(hist) - 1 if pos is None else pos, N, k)[0].tolist()
    # the tail [1, 2] was seen at columns 0 .. 1: what followed is 3, 1, 2 and then the draft itself
    assert d([1, 2, 3, 1, 2], 2, 5) == [3, 1, 2, 3, 1]
    # the same with unigrams only: the most recent earlier 2 is at column 1
    assert d([1, 2, 3, 1, 2], 1, 3) == [3, 1, 2]
    # an older LONGER match beats a newer shorter one: [7, 8, 9] at columns 0 .. 2 against the lone 9 at column 6
    assert d([7, 8, 9, 4, 5, 5, 9, 6, 7, 8, 9], 3, 3) == [4, 5, 5]
    assert d([7, 8, 9, 4, 5, 5, 9, 6, 7, 8, 9], 1, 3) == [6, 7, 8]
    # the most recent among equal lengths
    assert d([1, 2, 5, 1, 2, 6, 1, 2], 2, 2) == [6, 1]
    # no hit: the pending token repeated; one token: nothing to look up
    assert d([1, 2, 3, 4], 3, 3) == [4, 4, 4] and d([9], 3, 2) == [9, 9]
    # period 1: the hit ends at L - 2 and the draft feeds itself
    assert d([3, 5, 5], 2, 4) == [5, 5, 5, 5]
    # the n-gram may start at column 0 but not before it
    assert d([4, 6, 0, 4, 6], 8, 3) == [0, 4, 6]
    # position clamps: below 0 one token, beyond the columns all of them
    assert d([1, 2, 3, 1, 2], 2, 2, pos=-7) == [1, 1] and d([1, 2, 3, 1, 2], 2, 2, pos=99) == [3, 1]
    # only the first position + 1 columns are tokens
    assert d([1, 2, 3, 1, 2], 2, 2, pos=3) == [2, 3]


def _onehot(tokens, V):
    lg = np.zeros(tokens.shape + (V,), dtype=np.float16)
    np.put_along_axis(lg, np.asarray(tokens)[..., None], 1.0, axis=-1)
    return lg


def test_accept_reference_on_hand_written_cases():
    V, B, k = 16, 2, 3
    g = np.array([[5, 6, 7, 8], [1, 2, 3, 4]])
    lg = _onehot(g, V)
    state = lambda: dict(out_tokens=np.full((B, 6), -1), column=1, next_token=np.full(B, -1), position=10, limit=100,
                         hist=np.full((B, 13), -1), stats=np.array([2, 9]))

    def run(draft, **kw):
        s = dict(state(), **kw)
        return ref.spec_accept_ref(lg, np.array(draft), **s)

    # row 0 confirms 3 draft tokens, row 1 only 1: the minimum decides, n + 1 = 2 tokens are handed over
    out, col, tok, pos, hist, stats, adv = run([[5, 6, 7], [1, 9, 3]])
    assert adv == 2 and col == 3 and pos == 12 and stats.tolist() == [3, 11] and tok.tolist() == [6, 2]
    assert out.tolist() == [[-1, 5, 6, -1, -1, -1], [-1, 1, 2, -1, -1, -1]]
    assert hist[:, 11].tolist() == [5, 1] and hist[:, 12].tolist() == [6, 2] and (hist[:, :11] == -1).all()
    # everything confirmed: k + 1 tokens, the last two output columns lie outside the array and are skipped
    out, col, tok, pos, hist, stats, adv = run([[5, 6, 7], [1, 2, 3]], column=4)
    assert adv == 4 and col == 8 and pos == 14 and tok.tolist() == [8, 4] and out[:, 4:].tolist() == [[5, 6], [1, 2]]
    assert hist[:, 11:].tolist() == [[5, 6], [1, 2]]                       # history columns 13 and 14 do not exist
    # nothing confirmed: the plain greedy step
    assert run([[0, 6, 7], [1, 2, 3]])[6] == 1
    # the limit clamps; at or beyond it nothing but the step count moves
    assert run([[5, 6, 7], [1, 2, 3]], limit=3)[6] == 2
    out, col, tok, pos, hist, stats, adv = run([[5, 6, 7], [1, 2, 3]], limit=1)
    assert adv == 0 and col == 1 and pos == 10 and stats.tolist() == [3, 9] and (out == -1).all() and (tok == -1).all() and (hist == -1).all()
    assert run([[5, 6, 7], [1, 2, 3]], limit=-4)[6] == 0
    # the argmax rule: first index on ties, a NaN is the maximum, -0 == +0
    assert ref.greedy_token(np.array([1, 3, 3, 2], dtype=np.float16)) == 1
    assert ref.greedy_token(np.array([1, np.inf, np.nan, np.nan], dtype=np.float16)) == 2
    assert ref.greedy_token(np.array([-1, -0.0, 0.0], dtype=np.float16)) == 1
