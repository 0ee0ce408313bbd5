"""Few-row attention (eetq_decode_attention_rows_f16, eetq_amd/csrc/attn_decode_rows.hip) without a GPU: the C-ABI entry points
(declared, exported, refusing bad arguments before any launch), the two pure host functions, the chunk rule restated for every
(shape, splits) pair of tests/test_gpu_attn_rows.py, and the preconditions of every case that file runs -- each case is BUILT
here through tests/attn_cases.py: 200-unit gaps for the staircase and the pairing, a census that moves by more than its 1-ulp
tolerance when one row is lost or doubled, a rising ramp wherever the GPU file uses one, NaN behind `keys`."""
import ctypes
import os
import re

import numpy as np
import pytest

import attn_cases as ac
import test_gpu_attn_prefill_edges as edges
import test_gpu_attn_rows as rows
from conftest import ROOT

NEW_SYMBOLS = ("eetq_decode_attention_rows_f16", "eetq_decode_attention_rows_splits", "eetq_decode_attention_rows_max_splits",
               "eetq_decode_attention_rows_workspace_floats")
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
CAP = rows.MAX_SPLITS


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_new_symbols_are_declared_and_exported(lib):
    from eetq_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eetq_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.eetq_decode_attention_rows_max_splits() == CAP


def test_operator_names():
    import eetq_amd.ops as ops
    assert "decode_attention_rows" in ops.__all__ and "decode_attention_rows_splits" in ops.__all__
    if ops.BOUNDARY == "ext":
        assert callable(ops.decode_attention_rows) and callable(ops.decode_attention_rows_splits)
    else:
        assert ops.decode_attention_rows is None and ops.decode_attention_rows_splits is None


def test_workspace_formula(lib):
    f = lib.eetq_decode_attention_rows_workspace_floats
    for B, H, R, D, ns in ((2, 8, 5, 128, 3), (1, 40, 16, 128, 64), (4, 32, 1, 64, 1), (1, 2, 2, 64, 7)):
        assert f(B, H, R, D, ns) == B * H * R * ns * (D + 4)
    assert f(0, 8, 5, 128, 3) == 0 and f(2, 8, 5, 128, 0) == 0


def _call(lib, q=True, k=True, v=True, out=True, ws=True, st=True, B=1, H=4, Hkv=2, R=9, keys=340, D=128, splits=2, strides=None,
          ws_offset=0, kv_len=None):
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    arr = (ctypes.c_long * 12)(*(strides or [R * H * D, H * D, D, Hkv * 351 * D, 351 * D, D, Hkv * 351 * D, 351 * D, D, R * H * D, H * D, D]))
    return lib.eetq_decode_attention_rows_f16(p if q else None, p if k else None, p if v else None, p if out else None,
                                              ctypes.c_void_p(base + ws_offset) if ws else None, B, H, Hkv, R, keys, D, kv_len, 0, splits,
                                              ctypes.c_float(0.1), arr if st else None, None)


def test_refusals_without_a_gpu(lib):
    """every refusal returns before any launch: there is no GPU here, and the buffers are 4 KiB of host memory"""
    for missing in ("q", "k", "v", "out", "st"):
        assert _call(lib, **{missing: False}) == ERR_INVALID, missing
        assert b"null pointer" in lib.eetq_last_error()
    for R in (0, -1, 17):
        assert _call(lib, R=R) == ERR_INVALID and b"rows must lie in 1 .. 16" in lib.eetq_last_error()
    assert _call(lib, keys=0) == ERR_INVALID and b"max_keys" in lib.eetq_last_error()
    assert _call(lib, keys=-5) == ERR_INVALID
    for ns in (0, -2, CAP + 1):
        assert _call(lib, splits=ns) == ERR_INVALID and b"splits" in lib.eetq_last_error()
    assert _call(lib, ws=False) == ERR_INVALID and b"workspace" in lib.eetq_last_error()
    assert _call(lib, ws=False, splits=1) == ERR_INVALID and b"workspace" in lib.eetq_last_error()      # two launches at one chunk too
    assert _call(lib, ws_offset=4) == ERR_INVALID and b"workspace" in lib.eetq_last_error()
    assert _call(lib, D=96) == ERR_UNSUPPORTED and b"head_dim" in lib.eetq_last_error()
    assert _call(lib, H=3) == ERR_INVALID                                        # heads not a multiple of kv heads
    bad = [9 * 4 * 128, 4 * 128, 128, 2 * 351 * 128, 351 * 128, 132, 2 * 351 * 128, 351 * 128, 128, 9 * 4 * 128, 4 * 128, 128]
    assert _call(lib, strides=bad) == ERR_INVALID and b"strides" in lib.eetq_last_error()     # k rows 132 apart: not 16 bytes
    odd_out = [9 * 4 * 128, 4 * 128, 128, 2 * 351 * 128, 351 * 128, 128, 2 * 351 * 128, 351 * 128, 128, 9 * 4 * 128, 4 * 128 + 2, 128]
    assert _call(lib, strides=odd_out) == ERR_INVALID and b"strides" in lib.eetq_last_error()
    huge = [9 * 4 * 128, 4 * 128, 128, 2 * 351 * 128, 351 * 128, 1 << 24, 2 * 351 * 128, 351 * 128, 128, 9 * 4 * 128, 4 * 128, 128]
    assert _call(lib, strides=huge) == ERR_INVALID and b"2 GiB" in lib.eetq_last_error()      # checked against max_keys


def test_split_rule(lib):
    f = lib.eetq_decode_attention_rows_splits
    for B in (1, 2, 4, 16, 64):
        for H, Hkv in ((1, 1), (4, 2), (8, 2), (32, 8), (40, 40), (64, 8)):
            for R in (1, 2, 5, 16):
                for keys in (1, 31, 32, 33, 130, 340, 528, 1101, 4096, 16384, 1 << 20):
                    n = f(B, H, Hkv, R, keys)
                    assert 1 <= n <= CAP
                    blocks = -(-keys // rows.BLK)
                    assert n <= 32, "the rule stops at 32 chunks (64 can be forced)"
                    assert n == 1 or blocks // n >= (4 if n <= 8 else 8), "4 blocks per chunk up to 8 chunks, 8 beyond"
                    tiles, resident = -(-(H // Hkv * R) // 64), 2 if H // Hkv * R <= 16 else 1
                    assert n == 1 or n * B * Hkv * tiles <= resident * 256, "the grid fills the chip once"
                    sizes = [b - a for a, b in rows.chunks(keys, n)]
                    assert sum(sizes) == keys and min(sizes) > 0, "the rule leaves no chunk empty"
    # the measured corners (profiles/attn_rows.txt): the count that was fastest, or within the spread of it
    assert [f(1, 40, 40, 5, k + 5) for k in (1024, 4096, 16384)] == [8, 12, 12] and [f(4, 40, 40, 5, k + 5) for k in (1024, 4096, 16384)] == [3, 3, 3]
    assert [f(1, 32, 8, 3, k + 3) for k in (1024, 4096, 16384)] == [8, 16, 32] and [f(1, 32, 8, 9, k + 9) for k in (1024, 4096, 16384)] == [8, 16, 32]
    assert [f(4, 32, 8, 3, k + 3) for k in (1024, 4096, 16384)] == [8, 16, 16] and [f(4, 32, 8, 9, k + 9) for k in (1024, 4096, 16384)] == [8, 8, 8]
    assert f(0, 40, 40, 5, 2048) == 1 and f(1, 40, 40, 5, 0) == 1 and f(1, 40, 40, 0, 2048) == 1 and f(1, 40, 3, 5, 2048) == 1


def test_chunk_rule_covers_every_pair():
    rows.check_chunk_coverage()


def test_hot_rows_reach_what_they_claim():
    for s, n in rows.PAIRS:
        if s == rows.SHORT:
            continue
        ns = rows.default_splits(s) if n is None else n
        hot = set(rows.hot_rows(s, ns))
        koff = s.keys - s.T
        assert {0, s.keys - 1} <= hot and set(range(max(koff - 1, 0), s.keys)) <= hot, "the ends and the whole causal tail"
        for e in range(rows.BLK, s.keys, rows.BLK):
            assert {e - 1, e} <= hot, "both sides of every block edge"
        for a, b in rows.chunks(s.keys, ns):
            if 0 < a < s.keys and b > a:
                assert {a - 1, a} <= hot, "both sides of every chunk boundary"
        pairs = rows.two_step_pairs(s, ns)
        if s.keys > rows.BLK:
            assert any(a // rows.BLK != b // rows.BLK for a, b in pairs), "a two-step pair across a block edge"
        if s.T > 2:
            assert any(koff <= a < b for a, b in pairs), "a two-step pair inside the causal tail"
        starts = [a for a, b in rows.chunks(s.keys, ns) if 0 < a < s.keys and b > a]
        assert all((a - 1, a) in pairs for a in starts), "a two-step pair across every chunk boundary"


CASES = [(s, D) for s in rows.SHAPES for D in rows.DIMS]


@pytest.mark.parametrize("s,D", CASES, ids=[rows._id(s, None, D) for s, D in CASES])
def test_inputs_meet_their_preconditions(s, D):
    koff = s.keys - s.T
    if s != rows.SHORT:
        c = edges.staircase_case(s, D)
        assert ac.hot_gap(c["q1"], c["k"][:, :, : s.keys], c["hot"], c["scale"]) >= ac.GAP_MIN
        q64 = c["q1"].astype(np.float64)
        gap2 = ((q64 * c["hotter"].astype(np.float64)).sum(-1) - (q64 * c["hot"].astype(np.float64)).sum(-1)) * c["scale"]
        assert gap2.min() >= ac.GAP_MIN and (c["v"][:, :, : s.keys] != 0).all()
        assert np.isnan(c["k"][:, :, s.keys:]).all() and np.isnan(c["v"][:, :, s.keys:]).all() and c["k"].shape[2] == s.keys + ac.PREFILL_PAD
        for kind in ("diagonal", "permutation"):
            p = edges.pairing_case(s, D, kind)
            assert p["gap"] >= ac.GAP_MIN
            ref, _ = ac.prefill_reference(p["q"], p["k"], p["v"], s.keys, koff, p["scale"])
            assert not ac.check_pairing(ref.astype(np.float16), p).any()
    cen = edges.census_case(s, D)
    drop, dbl = ac.prefix_census_shift_ulps(cen["v"], ac.prefill_counts(s.T, s.keys, koff))
    assert drop > 1.0 and dbl > 1.0, (drop, dbl)
    assert np.isnan(cen["v"][:, :, s.keys:]).all()
    for scaling, ramp in rows.random_kinds(s):
        r = edges.random_case(s, D, scaling, ramp)       # raises when no rising ramp exists
        assert np.isfinite(r["k"][:, :, : s.keys].astype(np.float64)).all() and np.isnan(r["k"][:, :, s.keys:]).all()
        if ramp and s.keys > 64:
            assert (np.diff(ac.block_maxima(r["q"], r["k"], s.keys, koff, r["scale"]), axis=-1) > 0).all()
    assert (s == rows.NO_RAMP) == (len(rows.random_kinds(s)) == 2)
