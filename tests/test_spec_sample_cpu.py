"""Speculative decoding for sampled generation (eetq_spec_sample_accept_f16), everything that needs no GPU: the entry's surface in
the header, the library and both bindings, every argument refusal, and the NumPy reference (tests/spec_sample_ref.py) on
hand-written cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spec_ref
import spec_sample_ref as ref
from conftest import ROOT

ENTRY = "eetq_spec_sample_accept_f16"


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
    assert ENTRY in history                                     # listed among the entries added within revision 7
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % ENTRY, code)
    assert proto
    args = [a.strip() for a in proto.group(1).split(",")]
    accept = [a.strip() for a in re.search(r"\bint\s+eetq_spec_accept_f16\s*\(([^)]*)\)", code).group(1).split(",")]
    assert len(args) == 26 and args[:20] == accept[:20]         # eetq_spec_accept_f16's arguments, in its order, then ...
    assert args[20:] == ["const void* params", "int32_t* done", "const float* uniforms", "long uniforms_stride", "int64_t* workspace",
                         "void* stream"]
    assert hasattr(lib, ENTRY) and ENTRY in _lib.EXPORTED_SYMBOLS
    fn = getattr(lib, ENTRY)
    assert fn.argtypes is not None and len(fn.argtypes) == 26 and fn.restype is ctypes.c_int
    assert fn.argtypes[:20] == lib.eetq_spec_accept_f16.argtypes[:20]
    assert re.search(r"SRCS\s*:=.*\bspec_sample\.hip", open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read())


def test_bindings():
    from eetq_amd import ops, ops_ctypes
    assert "spec_sample_accept" in ops.__all__ and callable(ops.spec_sample_accept)
    assert "spec_sample_accept" in ops_ctypes.__all__ and callable(ops_ctypes.spec_sample_accept)
    z = torch.zeros(1, dtype=torch.int64)
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)
    for mod in (ops, ops_ctypes):                               # the checks run before any device work
        with pytest.raises(RuntimeError, match="float16 CUDA"):
            mod.spec_sample_accept(torch.zeros(1, 5, 8), i64(1, 4), i64(1, 4), z, z, z, z, i64(1, 8), i64(2),
                                   torch.zeros(8, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="float16 CUDA"):
            mod.spec_sample_accept(torch.zeros(1, 5, 8, dtype=torch.float16), i64(1, 4), i64(1, 4), z, z, z, z, i64(1, 8), i64(2),
                                   torch.zeros(8, dtype=torch.int32), None, None, i64(5))


def _buffer():
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 8 == 0
    return buf, p


def test_refusals_without_a_device(lib):
    buf, p = _buffer()
    good = dict(logits=p, stride_b=5 * 64, stride_t=64, vocab=64, batch=2, k=4, draft=p, draft_stride=4, out_tokens=p, out_stride=8,
                out_cols=8, column=p, position=p, limit=p, next_token=p, next_stride=1, hist=p, hist_stride=16, hist_cols=16,
                stats=p, params=p, done=p, uniforms=p, uniforms_stride=5, workspace=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.eetq_spec_sample_accept_f16(*[a[key] for key in good])

    # every refusal of eetq_spec_accept_f16 ...
    for arg in ("logits", "draft", "out_tokens", "column", "position", "limit", "next_token", "hist", "stats", "params", "workspace"):
        assert call(**{arg: None}) == -1
        assert arg.encode() in lib.eetq_last_error(), (arg, lib.eetq_last_error())
        if arg != "logits":
            assert call(**{arg: ctypes.c_void_p(p.value + 4)}) == -1
            assert b"aligned" in lib.eetq_last_error(), (arg, lib.eetq_last_error())
    assert call(logits=ctypes.c_void_p(p.value + 1)) == -1 and b"aligned" in lib.eetq_last_error()
    for arg, bad, word in (("k", 0, b"k must"), ("k", 16, b"k must"), ("vocab", 0, b"vocab"), ("vocab", -5, b"vocab"),
                           ("batch", 0, b"batch"), ("batch", -1, b"batch"), ("stride_t", 63, b"stride"), ("stride_b", 63, b"stride"),
                           ("draft_stride", 3, b"stride"), ("out_cols", 0, b"out_cols"), ("out_stride", 7, b"out_stride"),
                           ("hist_cols", 0, b"cols"), ("hist_stride", 15, b"stride"), ("next_stride", 0, b"next_token"),
                           # ... and its own: the uniforms' stride (only when they are given), the 24-bit ticket count
                           ("uniforms_stride", 4, b"uniforms"), ("batch", (1 << 24) // 5 + 1, b"2^24")):
        assert call(**{arg: bad}) == -1
        assert word in lib.eetq_last_error(), (arg, bad, lib.eetq_last_error())
    assert call(batch=1 << 20, k=15) == -1 and b"2^24" in lib.eetq_last_error()        # 2^20 * 16 = 2^24 exactly
    del buf


def _state(B, **kw):
    s = dict(out_tokens=np.full((B, 6), -1), column=1, next_token=np.full(B, -1), position=10, limit=100,
             hist=np.full((B, 13), -1), stats=np.array([2, 9]))
    s.update(kw)
    return s


def test_reference_objection_at_each_position():
    x = np.array([[5, 6, 7, 8], [1, 2, 3, 4]])
    for row in (0, 1):
        for j in range(3):
            draft = x[:, :3].copy()
            draft[row, j] += 1
            out, col, tok, pos, hist, stats, done, adv = ref.spec_sample_accept_ref(x, draft, **_state(2, hist=np.full((2, 16), -1)))
            assert adv == j + 1 and col == 1 + adv and pos == 10 + adv and stats.tolist() == [3, 9 + adv] and done is None
            assert tok.tolist() == x[:, j].tolist()
            assert out[:, 1:1 + adv].tolist() == x[:, :adv].tolist() and (out[:, 1 + adv:] == -1).all() and (out[:, 0] == -1).all()
            assert hist[:, 11:11 + adv].tolist() == x[:, :adv].tolist() and (hist[:, :11] == -1).all() and (hist[:, 11 + adv:] == -1).all()
    # no objection: k + 1 tokens; output columns 5 and 6 of 6 exist only in part, history columns 13 and 14 do not
    out, col, tok, pos, hist, stats, done, adv = ref.spec_sample_accept_ref(x, x[:, :3], **_state(2, column=3))
    assert adv == 4 and col == 7 and pos == 14 and tok.tolist() == [8, 4] and out[:, 3:].tolist() == [[5, 6, 7], [1, 2, 3]]
    assert hist[:, 11:].tolist() == [[5, 6], [1, 2]]


def test_reference_finished_rows_and_eos():
    x = np.array([[5, 6, 7, 8], [1, 2, 3, 4]])
    wrong = np.array([[5, 6, 7], [9, 9, 9]])
    # a row finished at entry hands on pads and never objects, whatever its draft says
    out, col, tok, pos, hist, stats, done, adv = ref.spec_sample_accept_ref(x, wrong, eos_token=40, pad_token=33, done=[0, 1],
                                                                            **_state(2))
    assert adv == 4 and out[:, 1:5].tolist() == [[5, 6, 7, 8], [33] * 4] and tok.tolist() == [8, 33] and done.tolist() == [0, 1]
    # done=None: nobody is finished at entry, row 1 objects at once
    assert ref.spec_sample_accept_ref(x, wrong, eos_token=40, pad_token=33, **_state(2))[7] == 1
    # an EOS at position 1 of row 1: the row is flagged, pads follow, its later mismatches do not end the step
    d = np.array([[5, 6, 7], [1, 2, 0]])
    out, col, tok, pos, hist, stats, done, adv = ref.spec_sample_accept_ref(x, d, eos_token=2, pad_token=33, done=[0, 0], **_state(2))
    assert adv == 4 and out[1, 1:5].tolist() == [1, 2, 33, 33] and done.tolist() == [0, 1] and tok.tolist() == [8, 33]
    # ... the EOS position itself does not object either (the row is finished AFTER it)
    d = np.array([[5, 6, 7], [1, 0, 0]])
    assert ref.spec_sample_accept_ref(x, d, eos_token=2, pad_token=33, done=[0, 0], **_state(2))[7] == 4
    # an EOS at position adv - 1 finishes the row: row 0 objects at position 1, where row 1 draws its EOS
    d = np.array([[5, 0, 7], [1, 2, 3]])
    out, col, tok, pos, hist, stats, done, adv = ref.spec_sample_accept_ref(x, d, eos_token=2, pad_token=33, done=[0, 0], **_state(2))
    assert adv == 2 and done.tolist() == [0, 1] and tok.tolist() == [6, 2] and out[:, 1:4].tolist() == [[5, 6, -1], [1, 2, -1]]
    # an EOS beyond adv finishes nothing: row 0 objects at position 0, row 1's EOS sits at position 1
    d = np.array([[0, 6, 7], [1, 2, 3]])
    out, col, tok, pos, hist, stats, done, adv = ref.spec_sample_accept_ref(x, d, eos_token=2, pad_token=33, done=[0, 0], **_state(2))
    assert adv == 1 and done.tolist() == [0, 0] and tok.tolist() == [5, 1]
    # every row finished: adv = want
    out, col, tok, pos, hist, stats, done, adv = ref.spec_sample_accept_ref(x, wrong, eos_token=2, pad_token=33, done=[1, 1],
                                                                            **_state(2, limit=4))
    assert adv == 3 and (out[:, 1:4] == 33).all() and done.tolist() == [1, 1]
    # eos_token < 0: no token finishes a row
    assert ref.spec_sample_accept_ref(x, np.array([[5, 6, 7], [1, 2, 0]]), eos_token=-1, done=[0, 0], **_state(2))[7] == 3


def test_reference_limit_clamps():
    x = np.array([[5, 6, 7, 8], [1, 2, 3, 4]])
    run = lambda limit, draft=x[:, :3]: ref.spec_sample_accept_ref(x, draft, done=[0, 0], **_state(2, limit=limit))
    for limit, adv in ((0, 0), (1, 0), (2, 1), (4, 3), (5, 4), (10, 4), (-4, 0)):
        assert run(limit)[7] == adv, limit
    out, col, tok, pos, hist, stats, done, adv = run(1)         # nothing but the step count moves
    assert col == 1 and pos == 10 and stats.tolist() == [3, 9] and (out == -1).all() and (tok == -1).all() and (hist == -1).all()
    assert done.tolist() == [0, 0]
    # the clamp wins over a later objection, an earlier objection over the clamp
    bad = x[:, :3].copy()
    bad[1, 2] = 0
    assert run(3, bad)[7] == 2 and run(10, bad)[7] == 3
    bad[0, 0] = 0
    assert run(3, bad)[7] == 1


def test_reference_draw_and_greedy_twin():
    """step 1 on rows whose answer is known, and T = 0 without EOS against the greedy reference (tests/spec_ref.py)"""
    rng = np.random.default_rng(0)
    lg = (rng.standard_normal((2, 4, 16)) * 2).astype(np.float16)
    g = np.array([[spec_ref.greedy_token(lg[b, t]) for t in range(4)] for b in range(2)])
    assert ref.draw_tokens(lg, 7, 4).tolist() == g.tolist()
    assert ref.draw_tokens(lg, 7, 2)[:, 2:].tolist() == [[-1, -1]] * 2          # positions >= want are not read
    assert ref.draw_tokens(lg, 7, 4, temperature=float("nan")).tolist() == g.tolist()
    for draft in (g[:, :3], np.array([[g[0, 0], 99, g[0, 2]], g[1, :3].tolist()])):
        a = spec_ref.spec_accept_ref(lg, draft, **_state(2))
        b = ref.spec_sample_accept_ref(ref.draw_tokens(lg, 1, 4), draft, **_state(2))
        assert all(np.array_equal(p, q) for p, q in zip(a[:6], b[:6])) and a[6] == b[7]
    flat = np.zeros((2, 3, 1001), dtype=np.float16)             # a flat row: token = floor(1001 u)
    u = [[0.0, 0.5, 1.5], [0.25, -1.0, 0.999]]
    assert ref.draw_tokens(flat, 0, 3, temperature=1.0, uniforms=u).tolist() == [[0, 500, 1000], [250, 0, 999]]
    import sampling_ref
    own = ref.draw_tokens(flat, 5, 3, temperature=0.7, seed=9)
    assert own.tolist() == [[int(np.float64(sampling_ref.philox_uniform(9, 5 + t, b)) * 1001) for t in range(3)] for b in range(2)]
