"""Ragged (left-padded) batches without a GPU: the three C-ABI entries with a per-row first key (declared, exported, prototyped,
refusing bad arguments before any launch with the messages of their twins), the ``kv_start`` keyword of both bindings, the
``padded_static_batch`` promise of the attention modules, and ``left_pad_starts``, the pure check of a left-padded mask that
``GraphDecoder(ragged=True)`` runs on its ``attention_mask``."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

NEW_SYMBOLS = ("eetq_prefill_attention_padded_f16", "eetq_decode_attention_padded_f16", "eetq_rope_decode_attention_padded_f16")
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_new_symbols_are_declared_exported_and_prototyped(lib):
    from eetq_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eetq_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
        twin = getattr(lib, {"eetq_prefill_attention_padded_f16": "eetq_prefill_attention_dev_f16",
                             "eetq_decode_attention_padded_f16": "eetq_decode_attention_f16",
                             "eetq_rope_decode_attention_padded_f16": "eetq_rope_decode_attention_bounded_f16"}[name])
        assert len(fn.argtypes) == len(twin.argtypes) + 1                       # the twin plus kv_start
    assert lib.eetq_abi_version() == 7


def _buf():
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return buf, ctypes.c_void_p(base)


def _prefill(lib, start=True, q=True, st=True, H=4, Hkv=2, T=40, keys=340, D=128, splits=2, strides=None, padded=True):
    buf, p = _buf()
    arr = (ctypes.c_long * 12)(*(strides or [T * H * D, H * D, D, Hkv * 351 * D, 351 * D, D, Hkv * 351 * D, 351 * D, D, T * H * D, H * D, D]))
    head = (p if q else None, p, p, p, p, 1, H, Hkv, T, keys, D, None, 0)
    tail = (splits, ctypes.c_float(0.1), arr if st else None, None)
    if padded:
        return lib.eetq_prefill_attention_padded_f16(*head, p if start else None, *tail)
    return lib.eetq_prefill_attention_dev_f16(*head, *tail)


def _decode(lib, start=True, q=True, H=4, Hkv=2, S=64, D=128, strides=None, padded=True):
    buf, p = _buf()
    arr = (ctypes.c_long * 11)(*(strides or [H * D, D, Hkv * S * D, S * D, D, Hkv * S * D, S * D, D, 0, H * D, D]))
    head = (p if q else None, p, p, None, p, p, 1, H, Hkv, S, D, 2, ctypes.c_float(0.1), arr, None, 0)
    if padded:
        return lib.eetq_decode_attention_padded_f16(*head, p if start else None, None, None)
    return lib.eetq_decode_attention_f16(*head, None, None)


def _rope(lib, start=True, q=True, H=4, Hkv=2, S=64, D=128, strides=None, padded=True):
    buf, p = _buf()
    arr = (ctypes.c_long * 12)(*(strides or [H * D, Hkv * D, Hkv * D, Hkv * S * D, S * D, D, Hkv * S * D, S * D, D, 0, H * D, D]))
    head = (p, None, 0, p if q else None, p, p, p, 16, p, p, None, p, p, p, 1, H, Hkv, S, D, 2, ctypes.c_float(0.1), arr, None, 0)
    if padded:
        return lib.eetq_rope_decode_attention_padded_f16(*head, p if start else None, None, None)
    return lib.eetq_rope_decode_attention_bounded_f16(*head, None, None)


@pytest.mark.parametrize("call", (_prefill, _decode, _rope), ids=("prefill", "decode", "rope_decode"))
def test_refusals_before_any_launch(lib, call):
    """No GPU here: every one of these must come back before a launch is attempted, and say what its twin says."""
    assert call(lib, start=False) == ERR_INVALID and b"kv_start" in lib.eetq_last_error()

    def same(**kw):
        want = call(lib, padded=False, **kw)
        msg = lib.eetq_last_error()
        assert want != 0
        assert call(lib, **kw) == want and lib.eetq_last_error() == msg, (kw, msg)
        return want, msg

    assert same(q=False) == (ERR_INVALID, lib.eetq_last_error()) and b"null pointer" in lib.eetq_last_error()
    assert same(D=96)[0] == ERR_UNSUPPORTED                                    # bad head size
    assert same(H=3)[0] == ERR_INVALID                                         # heads not a multiple of kv heads
    if call is _prefill:
        bad = [40 * 4 * 128, 4 * 128, 128, 2 * 351 * 128, 351 * 128, 132, 2 * 351 * 128, 351 * 128, 128, 40 * 4 * 128, 4 * 128, 128]
        assert same(strides=bad)[0] == ERR_INVALID and b"strides" in lib.eetq_last_error()
        assert same(st=False)[0] == ERR_INVALID
        assert same(splits=17)[0] == ERR_INVALID and b"splits" in lib.eetq_last_error()
        assert same(keys=0)[0] == ERR_INVALID and b"max_keys" in lib.eetq_last_error()
    elif call is _decode:
        bad = [4 * 128, 128, 2 * 64 * 128, 64 * 128, 132, 2 * 64 * 128, 64 * 128, 128, 0, 4 * 128, 128]
        assert same(strides=bad)[0] == ERR_INVALID and b"strides" in lib.eetq_last_error()
    else:
        bad = [4 * 128, 2 * 128, 2 * 128, 2 * 64 * 128, 64 * 128, 132, 2 * 64 * 128, 64 * 128, 128, 0, 4 * 128, 128]
        assert same(strides=bad)[0] == ERR_INVALID and b"strides" in lib.eetq_last_error()


def test_kv_start_keyword_in_both_bindings():
    import eetq_amd.ops_ctypes as oc
    for name in ("decode_attention", "rope_decode_attention"):
        p = inspect.signature(getattr(oc, name)).parameters
        assert "kv_start" in p and p["kv_start"].default is None, name
    from eetq_amd import _ext
    mod = _ext.load()
    for name in ("prefill_attention", "decode_attention", "rope_decode_attention"):
        assert re.search(r"kv_start: [^=]*= None", getattr(mod, name).__doc__), name
    import eetq_amd.ops as ops
    if ops.BOUNDARY == "ext":
        assert ops.prefill_attention is mod.prefill_attention and ops.decode_attention is mod.decode_attention


def test_kv_start_is_checked_before_launch():
    """int64 [B], contiguous, on the query's device -- anything else raises in the binding (CPU tensors: nothing can launch)."""
    import eetq_amd.ops_ctypes as oc
    q = torch.zeros(2, 4, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="kv_start"):
        oc._check_kv_start("decode_attention", torch.zeros(2, dtype=torch.int32), q, 2)
    with pytest.raises(RuntimeError, match="kv_start"):
        oc._check_kv_start("decode_attention", torch.zeros(3, dtype=torch.int64), q, 2)
    with pytest.raises(RuntimeError, match="kv_start"):
        oc._check_kv_start("decode_attention", torch.zeros(4, dtype=torch.int64)[::2], q, 2)
    with pytest.raises(RuntimeError, match="kv_start"):
        oc._check_kv_start("decode_attention", [0, 0], q, 2)
    oc._check_kv_start("decode_attention", torch.zeros(2, dtype=torch.int64), q, 2)


def test_padded_static_batch_is_exported_and_thread_local():
    import threading
    import eetq_amd.modules.llama_modules as lm
    assert "padded_static_batch" in lm.__all__
    starts = torch.tensor([2, 0])
    seen = []
    assert lm._padded_starts() is None
    with lm.padded_static_batch(starts):
        assert lm._padded_starts() is starts
        t = threading.Thread(target=lambda: seen.append(lm._padded_starts()))
        t.start()
        t.join()
        with lm.padded_static_batch(None):
            assert lm._padded_starts() is None
        assert lm._padded_starts() is starts
    assert lm._padded_starts() is None and seen == [None]


def test_left_pad_starts():
    from eetq_amd.utils.graph_decoder import left_pad_starts
    s = left_pad_starts(torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1]]))
    assert s.dtype == torch.int64 and s.tolist() == [2, 0]
    assert left_pad_starts(torch.tensor([[False, True], [True, True]])).tolist() == [1, 0]
    assert left_pad_starts(torch.tensor([[0, 0, 0, 7]], dtype=torch.int32)).tolist() == [3]
    for bad, what in (([[0, 1, 0, 1], [1, 1, 1, 1]], "left-padded"),        # a hole
                      ([[1, 1, 1, 1], [1, 1, 0, 0]], "left-padded"),        # right padding
                      ([[0, 0, 0, 0], [1, 1, 1, 1]], "at least one"),       # an all-pad row
                      ([1, 1, 1, 1], r"\[batch, P\]"),                       # not 2-D
                      ([[[1, 1]]], r"\[batch, P\]")):
        with pytest.raises(ValueError, match=what):
            left_pad_starts(torch.tensor(bad))
    with pytest.raises(ValueError, match="keep flags"):
        left_pad_starts(torch.zeros(2, 3))                                     # an additive float mask is not keep flags
