"""The device-length and split-KV forms of the prompt-attention kernel without a GPU: the new C-ABI entry points (declared,
exported, refusing bad arguments before any launch), the host-side split rule, and a NumPy emulation of the split arithmetic
(every share's running (m, l, o) over its own key blocks in the kernel's fp32 / fp16 steps, then the merge: weights
exp2(m_i - max m), one division) that goes through the family drivers of tests/test_gpu_attn_prefill_edges.py at the split
shapes of tests/test_gpu_attn_prefill_append.py and passes them, while three mutants each fail one.  The inputs' preconditions
(200-unit gaps, the census's sensitivity, rising block maxima) are proved here for those shapes.

The third mutant is an empty share that reports (m, l) = (0, 1), the state of a softmax that has seen one key of score 0.  An
empty share reporting l = 1 next to m = -inf cannot be seen in any output: its weight exp2(-inf) is exactly 0, so the merge never
reads its l (test_an_empty_share_with_minus_infinity_has_no_weight)."""
import ctypes
import os
import re

import numpy as np
import pytest

import attn_cases as ac
import test_attn_prefill_cases_cpu as cases
import test_gpu_attn_prefill_append as app
import test_gpu_attn_prefill_edges as edges
from conftest import ROOT

NEW_SYMBOLS = ("eetq_prefill_attention_dev_f16", "eetq_prefill_attention_splits", "eetq_prefill_attention_max_splits",
               "eetq_prefill_attention_workspace_floats")
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
CAP = 16


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


# ---- the library -------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_and_exported(lib):
    from eetq_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eetq_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.eetq_abi_version() == 7
    assert lib.eetq_prefill_attention_max_splits() == CAP
    assert lib.eetq_prefill_attention_workspace_floats(2, 8, 40, 128, 3) == 2 * 8 * 40 * 3 * 130
    assert lib.eetq_prefill_attention_workspace_floats(2, 8, 40, 128, 1) == 0


def _call(lib, q=True, k=True, v=True, out=True, ws=True, st=True, B=1, H=4, Hkv=2, T=40, keys=340, D=128, splits=2, strides=None,
          ws_offset=0, kv_len=None):
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    arr = (ctypes.c_long * 12)(*(strides or [T * H * D, H * D, D, Hkv * 351 * D, 351 * D, D, Hkv * 351 * D, 351 * D, D, T * H * D, H * D, D]))
    return lib.eetq_prefill_attention_dev_f16(p if q else None, p if k else None, p if v else None, p if out else None,
                                              ctypes.c_void_p(base + ws_offset) if ws else None, B, H, Hkv, T, keys, D, kv_len, 0, splits,
                                              ctypes.c_float(0.1), arr if st else None, None)


def test_refusals_without_a_gpu(lib):
    for missing in ("q", "k", "v", "out", "st"):
        assert _call(lib, **{missing: False}) == ERR_INVALID, missing
        assert b"null pointer" in lib.eetq_last_error()
    assert _call(lib, splits=0) == ERR_INVALID and b"splits" in lib.eetq_last_error()
    assert _call(lib, splits=-2) == ERR_INVALID
    assert _call(lib, splits=CAP + 1) == ERR_INVALID and b"splits" in lib.eetq_last_error()
    assert _call(lib, ws=False) == ERR_INVALID and b"workspace" in lib.eetq_last_error()
    assert _call(lib, ws_offset=4) == ERR_INVALID and b"workspace" in lib.eetq_last_error()
    assert _call(lib, keys=0) == ERR_INVALID and b"max_keys" in lib.eetq_last_error()
    assert _call(lib, keys=-5, splits=1, ws=False) == ERR_INVALID
    assert _call(lib, D=96) == ERR_UNSUPPORTED
    assert _call(lib, H=3) == ERR_INVALID                                        # heads not a multiple of kv heads
    bad = [40 * 4 * 128, 4 * 128, 128, 2 * 351 * 128, 351 * 128, 132, 2 * 351 * 128, 351 * 128, 128, 40 * 4 * 128, 4 * 128, 128]
    assert _call(lib, strides=bad) == ERR_INVALID and b"strides" in lib.eetq_last_error()     # k rows 132 apart: not 16 bytes
    huge = [40 * 4 * 128, 4 * 128, 128, 2 * 351 * 128, 351 * 128, 1 << 24, 2 * 351 * 128, 351 * 128, 128, 40 * 4 * 128, 4 * 128, 128]
    assert _call(lib, strides=huge) == ERR_INVALID and b"2 GiB" in lib.eetq_last_error()      # checked against max_keys


def test_split_rule(lib):
    f = lib.eetq_prefill_attention_splits
    for B in (1, 4):
        for T in (1024, 2048, 4096):
            for keys in (T, T + 4096):
                assert f(B, 40, T, keys) == 1, "q_tokens >= 1024 at 40 heads fill the chip by themselves"
    for B in (1, 2, 4, 16, 64):
        for H in (1, 4, 8, 32, 40, 64):
            for T in (1, 16, 64, 128, 129, 512, 1024):
                for keys in (1, 63, 64, 65, 130, 340, 512, 2048, 4096, 16384, 1 << 20):
                    n = f(B, H, T, keys)
                    assert 1 <= n <= CAP
                    assert n <= -(-keys // 64), "more shares than key blocks"
                    if 4 * 2 * -(-T // 128) * H * B > 5 * 256:           # two shares would pass 1.25 workgroups per compute unit
                        assert n == 1
    # the measured corners (profiles/prefill_attn_append.txt): splits where the table shows a gain, 1 where it shows none
    assert [f(1, 40, 64, k + 8) for k in (576, 2112, 4160)] == [2, 4, 4] and [f(4, 40, 64, k + 8) for k in (576, 2112, 4160)] == [1, 2, 2]
    assert [f(1, 32, 128, k + 8) for k in (640, 2176, 4224)] == [2, 4, 8] and [f(4, 32, 128, k + 8) for k in (640, 2176, 4224)] == [1, 2, 2]
    assert [f(1, 40, 512, k + 8) for k in (1024, 2560, 4608)] == [1, 2, 2] and f(4, 40, 512, 4616) == 1
    assert f(0, 40, 16, 2048) == 1 and f(1, 40, 16, 0) == 1 and f(1, 40, -1, 2048) == 1


# ---- the emulation -------------------------------------------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def emulate_split(q, k, v, keys, koff, scale, ns, mutant=None):
    """The split form on NumPy arrays (see tests/test_attn_prefill_cases_cpu.py::emulate for the unsplit arithmetic, which this
    repeats per share): q [B, T, H, D], k, v [B, Hkv, S, D] fp16 -> fp16 [B, T, H, D]."""
    B, T, H, D = q.shape
    Hkv = k.shape[1]
    koff = keys - T if koff is None else koff
    c = np.float32(np.float32(D ** -0.5 if scale is None else scale) * cases.LOG2E)
    hk = np.arange(H) // (H // Hkv)
    nb_all = -(-keys // 64)
    kk = np.zeros((B, Hkv, max(nb_all, 1) * 64, D), dtype=np.float32)
    vv = np.zeros_like(kk)
    kk[:, :, :keys], vv[:, :, :keys] = k[:, :, :keys], v[:, :, :keys]
    kk, vv = kk[:, hk], vv[:, hk]
    qf = q.astype(np.float32).transpose(0, 2, 1, 3)
    t = np.arange(T)
    q0, w0 = (t // 128) * 128, (t // 32) * 32
    kend = np.minimum(keys, q0 + 128 + koff)
    nblk = np.where(kend > 0, -(-kend // 64), 0)
    recs = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(ns):
            j0, j1 = i * nblk // ns, (i + 1) * nblk // ns
            if mutant == "shifted_boundary" and i == 1:          # share 1 starts a block late: the block is lost
                j0 = np.minimum(j0 + 1, j1)
            if mutant == "doubled_boundary" and i == 0:          # share 0 ends a block late: the block is counted twice
                j1 = np.minimum(j1 + 1, nblk)
            m = np.full((B, H, T), -np.inf, dtype=np.float32)
            l = np.zeros((B, H, T), dtype=np.float32)
            o = np.zeros((B, H, T, D), dtype=np.float32)
            for j in range(nb_all):
                key0 = j * 64
                key = key0 + np.arange(64)
                run = (j >= j0) & (j < j1) & (key0 <= w0 + 31 + koff)
                if not run.any():
                    continue
                valid = (key[None, :] <= (t + koff)[:, None]) & (key[None, :] < keys)
                s = np.matmul(qf, kk[:, :, key0: key0 + 64].transpose(0, 1, 3, 2))
                s = np.where(~valid, np.float32(-np.inf), s)
                mloc = _f32(s.max(-1).astype(np.float64) * np.float64(c) - np.float64(cases.P_SHIFT))
                m_new = np.maximum(m, mloc)
                m_use = np.where(m_new > -np.inf, m_new, np.float32(0))
                alpha = _f32(np.exp2((m - m_use).astype(np.float64)))
                p = _f32(np.exp2(s.astype(np.float64) * np.float64(c) - m_use[..., None].astype(np.float64)))
                p = np.where(np.isnan(p), np.float32(0), p)
                l_new = l * alpha + p.sum(-1, dtype=np.float32)
                o_new = o * alpha[..., None] + np.matmul(p.astype(np.float16).astype(np.float32), vv[:, :, key0: key0 + 64])
                m, l, o = np.where(run, m_new, m), np.where(run, l_new, l), np.where(run[:, None], o_new, o)
            if mutant == "empty_reports_one":
                empty = np.broadcast_to(j1 <= j0, m.shape)
                m, l = np.where(empty, np.float32(0), m), np.where(empty, np.float32(1), l)
            if mutant == "empty_l_one_only":
                l = np.where(np.broadcast_to(j1 <= j0, m.shape), np.float32(1), l)
            recs.append((m, l, o))
        # ---- the merge ----
        top = np.maximum.reduce([m for m, _, _ in recs])
        m_use = np.where(top > -np.inf, top, np.float32(0))
        L = np.zeros((B, H, T), dtype=np.float64)
        O = np.zeros((B, H, T, D), dtype=np.float64)
        for m, l, o in recs:
            w = _f32(np.exp2((m - m_use).astype(np.float64)))
            if mutant == "unweighted_merge":
                w = np.ones_like(w)
            L = _f32(w.astype(np.float64) * l + L).astype(np.float64)                 # fma, rounded to fp32
            O = _f32(w[..., None].astype(np.float64) * o + O).astype(np.float64)
        L, O = L.astype(np.float32), O.astype(np.float32)
        inv = np.where(L > 0, np.float32(1) / np.where(L > 0, L, np.float32(1)), np.float32(0))
        return (O * inv[..., None]).astype(np.float16).transpose(0, 2, 1, 3).copy()


def emu(ns, mutant=None):
    return lambda q, k, v, keys, koff, scale: emulate_split(q, k, v, keys, koff, scale, ns, mutant)


def test_one_share_is_the_unsplit_emulation():
    s, D = app.ROW2, 64
    c = edges.random_case(s, D, "one", True)
    a = emulate_split(c["q"], c["k"], c["v"], s.keys, s.koff, 1.0, 1)
    b = cases.emulate(c["q"], c["k"], c["v"], s.keys, s.koff, 1.0)
    assert np.array_equal(a.view(np.int16), b.view(np.int16))


def test_split_coverage_guard_holds():
    app.check_split_coverage()


@pytest.mark.parametrize("i,D", app.CASES, ids=app.CASE_IDS)
def test_inputs_meet_their_preconditions(i, D):
    """What the GPU assertions at the split shapes rest on: the staircase's and the pairing's 200-unit gaps, a census that moves
    by more than 3 ulp when any one row is dropped or doubled, block maxima that rise under the ramp, NaN behind `keys`."""
    s, _ = app.SPLIT[i]
    koff = edges.koff_of(s)
    c = edges.staircase_case(s, D)
    assert ac.hot_gap(c["q1"], c["k"][:, :, : s.keys], c["hot"], c["scale"]) >= ac.GAP_MIN
    q64 = c["q1"].astype(np.float64)
    gap2 = ((q64 * c["hotter"].astype(np.float64)).sum(-1) - (q64 * c["hot"].astype(np.float64)).sum(-1)) * c["scale"]
    assert gap2.min() >= ac.GAP_MIN and (c["v"][:, :, : s.keys] != 0).all()
    assert np.isnan(c["k"][:, :, s.keys:]).all() and np.isnan(c["v"][:, :, s.keys:]).all() and c["k"].shape[2] == s.keys + ac.PREFILL_PAD
    if s.koff is None:
        for kind in ("diagonal", "permutation"):
            p = edges.pairing_case(s, D, kind)
            assert ac.pairing_gap(p["q0"], p["k"], p["pi"], s.keys, koff, p["scale"]) >= ac.GAP_MIN
            ref, _ = ac.prefill_reference(p["q"], p["k"], p["v"], s.keys, koff, p["scale"])
            assert not ac.check_pairing(ref.astype(np.float16), p).any()
    cen = edges.census_case(s, D)
    drop, dbl = ac.prefix_census_shift_ulps(cen["v"], ac.prefill_counts(s.T, s.keys, koff))
    assert drop > 3.0 and dbl > 3.0, (drop, dbl)
    for scaling in ("default", "one"):
        r = edges.random_case(s, D, scaling, True)
        bm = ac.block_maxima(r["q"], r["k"], s.keys, koff, r["scale"])
        assert (np.diff(bm, axis=-1) > 0).all() and np.isfinite(r["k"][:, :, : s.keys].astype(np.float64)).all()


@pytest.mark.parametrize("i,D", app.CASES, ids=app.CASE_IDS)
def test_emulation_passes_every_family(i, D):
    s, ns = app.SPLIT[i]
    edges.drive_staircase_edges(emu(ns), s, D)
    if s.koff is None:
        edges.drive_pairing(emu(ns), s, D, "diagonal")
        edges.drive_pairing(emu(ns), s, D, "permutation")
    ulp = edges.drive_census(emu(ns), s, D)
    ratios = [edges.drive_random(emu(ns), s, D, scaling, ramp) for scaling, ramp in edges.RANDOM_KINDS]
    print("prefill-append emulation %s D=%d: census %.4f ulp, random %s" % (app.SPLIT_IDS[i], D, ulp, ["%.3f" % r for r in ratios]))


A3, A4, B8 = app.SPLIT[1], app.SPLIT[2], app.SPLIT[3]
MUTANTS = {
    # name: [(driver, (shape, splits), further arguments)] -- every listed run must fail, at both head sizes
    "unweighted_merge": [(edges.drive_staircase_edges, A3, ()), (edges.drive_random, A3, ("default", True)),
                         (edges.drive_pairing, A4, ("diagonal",))],
    "shifted_boundary": [(edges.drive_census, A3, ()), (edges.drive_staircase_edges, A3, ()), (edges.drive_census, A4, ())],
    "doubled_boundary": [(edges.drive_census, A3, ()), (edges.drive_census, A4, ())],
    "empty_reports_one": [(edges.drive_census, B8, ()), (edges.drive_random, B8, ("default", False))],
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
@pytest.mark.parametrize("D", edges.DIMS)
def test_mutant_is_caught(name, D):
    for fn, (s, ns), extra in MUTANTS[name]:
        assert cases._fails(fn, emu(ns, name), s, D, *extra), "%s passes %s on %s at D = %d" % (name, fn.__name__, s, D)


def test_an_empty_share_with_minus_infinity_has_no_weight():
    """(m, l) = (-inf, 1) from an empty share changes no bit: the merge multiplies its l by exp2(-inf) = 0."""
    s, ns = B8
    c = edges.census_case(s, 64)
    a = emulate_split(c["q"], c["k"], c["v"], s.keys, s.koff, None, ns)
    b = emulate_split(c["q"], c["k"], c["v"], s.keys, s.koff, None, ns, "empty_l_one_only")
    assert np.array_equal(a.view(np.int16), b.view(np.int16))
