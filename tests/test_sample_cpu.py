"""Sampling decode hand-over (eetq_sample_handover_f16), everything that needs no GPU: the entry's surface in the header, the
library and both bindings, its refusals, the parameter block's layout, Philox known answers, and the NumPy reference
(tests/sampling_ref.py) pinned to transformers' logits warpers on the CPU."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import sampling_ref as ref
from conftest import ROOT

NAME = "eetq_sample_handover_f16"


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_entry_surface(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, code)
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr and lib.eetq_abi_version() == 7
    assert hasattr(lib, NAME) and NAME in _lib.EXPORTED_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == 14 and fn.restype is ctypes.c_int
    assert "sample.hip" in open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()


def test_refusals_without_a_device(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 8 == 0
    good = dict(logits=p, row_stride=64, vocab=64, batch=2, out_tokens=p, out_stride=8, out_cols=8, column=p, next_token=p,
                position=p, params=p, done=None, uniforms=None, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.eetq_sample_handover_f16(*[a[k] for k in good])

    for arg in ("logits", "out_tokens", "column", "next_token", "position", "params"):
        assert call(**{arg: None}) == -1
        assert arg.encode() in lib.eetq_last_error(), (arg, lib.eetq_last_error())
    for arg, bad in (("vocab", 0), ("vocab", -3), ("batch", -1), ("row_stride", 63), ("out_cols", 0), ("out_stride", 7)):
        assert call(**{arg: bad}) == -1
        assert arg.encode() in lib.eetq_last_error(), (arg, lib.eetq_last_error())
    assert call(params=ctypes.c_void_p(p.value + 4)) == -1
    assert b"params" in lib.eetq_last_error() and b"aligned" in lib.eetq_last_error()
    assert call(batch=0) == 0                      # nothing to do: OK without a launch


def test_bindings_and_parameter_block():
    from eetq_amd import ops, ops_ctypes, sampling
    assert "sample_handover" in ops.__all__ and callable(ops.sample_handover)
    assert "sample_handover" in ops_ctypes.__all__ and callable(ops_ctypes.sample_handover)
    assert ops.sampling_params is sampling.sampling_params
    raw = sampling.pack_sampling_params(temperature=0.8, top_k=50, top_p=0.9, seed=2 ** 63 + 5, eos_token_id=2, pad_token_id=7)
    assert len(raw) == 32
    t, p, k, eos, pad, rsv, seed = struct.unpack("<ffiiiiQ", raw)
    assert (t, p) == (np.float32(0.8), np.float32(0.9)) and (k, eos, pad, rsv, seed) == (50, 2, 7, 0, 2 ** 63 + 5)
    blk = sampling.sampling_params(device="cpu")
    assert blk.dtype == torch.int32 and blk.shape == (8,)
    assert struct.unpack("<ffiiiiQ", blk.numpy().tobytes()) == (1.0, 1.0, 0, -1, 0, 0, 0)
    same = sampling.sampling_params(temperature=0.0, top_k=3, eos_token_id=11, out=blk)
    assert same is blk and struct.unpack("<ffiiiiQ", blk.numpy().tobytes()) == (0.0, 1.0, 3, 11, 0, 0, 0)
    with pytest.raises(ValueError):
        sampling.sampling_params(out=torch.zeros(8))
    for mod in (ops, ops_ctypes):                 # the checks run before any device work
        with pytest.raises(RuntimeError, match="float16 CUDA"):
            z = torch.zeros(1, dtype=torch.int64)
            mod.sample_handover(torch.zeros(1, 8), torch.zeros(1, 4, dtype=torch.int64), z, z, z, blk)


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        assert " ".join("%08x" % x for x in ref.philox4x32_10(ctr, key)) == want
    u = ref.philox_uniform(2 ** 63 + 5, 2 ** 32 + 3, 1)
    x0 = ref.philox4x32_10((3, 1, 1, 0), (5, 0x80000000))[0]
    assert 0.0 <= u < 1.0 and u == np.float32((x0 >> 8) / 2.0 ** 24)


def _distinct_row(seed, V=1001):
    """a random permutation of V distinct fp16 values in (-6, 6)"""
    rng = np.random.default_rng(seed)
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    vals = bits.view(np.float16)
    vals = vals[np.isfinite(vals) & (np.abs(vals.astype(np.float32)) < 6.0) & (vals != 0)]
    return rng.permutation(rng.choice(vals, V, replace=False))


@pytest.mark.parametrize("k", [1, 50, 1000])
@pytest.mark.parametrize("p", [0.1, 0.9])
def test_reference_equals_transformers_warpers(k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    T = 0.7
    row = _distinct_row(3)
    assert np.unique(row).size == row.size == 1001
    r = ref.sample_row(row, T, top_k=k, top_p=p)
    assert r.p_margin >= 2.0 ** -12, r.p_margin          # p is 2^-12 away from every cut: fp32 against fp64 cannot differ
    scores = torch.from_numpy(row.astype(np.float32))[None]
    for warper in (TemperatureLogitsWarper(T), TopKLogitsWarper(k), TopPLogitsWarper(p)):
        scores = warper(None, scores)
    assert np.array_equal(torch.isfinite(scores[0]).numpy(), r.kept)
    # the ordered survivors and their intervals: descending values, intervals that tile [0, 1)
    assert np.all(np.diff(row[r.order].astype(np.float64)) < 0) and r.lo[0] == 0.0 and abs(r.hi[-1] - 1.0) < 1e-12
    assert r.token(0.0) == r.order[0] and r.token(np.nextafter(1.0, 0.0)) == r.order[-1] and r.token(1.0) == r.order[-1]
    prob = torch.softmax(scores[0].double(), -1).numpy()
    assert np.allclose((r.hi - r.lo), prob[r.order], rtol=0, atol=1e-6)


def test_reference_keeps_a_tie_that_straddles_the_cut():
    # classes (descending): 4.0 alone, then 3.0 three times, then 1.0; at T = 1 the masses are ~0.46, 3 x 0.17, 0.02
    row = np.array([1.0, 3.0, 4.0, 3.0, -2.0, 3.0], dtype=np.float16)
    r = ref.sample_row(row, 1.0, top_p=0.7)               # 0.46 < 0.7 < 0.46 + 0.17: the cut falls inside the tie
    assert r.kept.tolist() == [False, True, True, True, False, True] and r.p_margin > 2.0 ** -12
    assert r.order.tolist() == [2, 1, 3, 5]
    assert r.token((r.lo[3] + r.hi[3]) / 2) == 5
    r = ref.sample_row(row, 1.0, top_k=2)                 # the 2nd and 3rd values are equal: ties at the threshold all stay
    assert r.order.tolist() == [2, 1, 3, 5]
    # NaN counts as -inf, -inf is never kept, +inf wins, an all -inf row gives 0
    r = ref.sample_row(np.array([np.nan, 1.0, -np.inf, 1.0], dtype=np.float16), 1.3)
    assert r.order.tolist() == [1, 3] and r.token(0.75) == 3
    assert ref.sample_row(np.array([1.0, np.inf, np.nan, np.inf], dtype=np.float16), 1.0).token(0.9) == 1
    assert ref.sample_row(np.array([-np.inf, np.nan], dtype=np.float16), 1.0).token(0.5) == 0
    assert ref.greedy_token(np.array([1.0, np.inf, np.nan, np.nan], dtype=np.float16)) == 2
