"""Few-row attention behind int8 cache rows (eetq_decode_attention_rows_i8kv_f16, the KV8 instantiations of
eetq_amd/csrc/attn_decode_rows.hip) without a GPU: the new C-ABI entry (declared, exported, ABI still 7, refusing bad arguments before
any launch), the operator's name on both boundaries, the ``few_rows_int8`` promise of llama_modules, the preconditions of every case
tests/test_gpu_attn_rows_i8kv.py runs -- each case is BUILT here: the 200-unit gaps after quantisation, a census that moves by more
than its 1-ulp tolerance when a row is lost or doubled, the 0x80 / NaN pad -- and a NumPy emulation of the new arithmetic: K bytes as
exact integers, (ks * scaling log2 e) * (q . k8) in fp32 per key before the mask select, V rows as fp16(vs * v8), p rounded to fp16 at
2^12, 32-key blocks dealt to four waves inside the chunks of the CHUNK RULE, the waves' states merged in wave order into the chunk's
record, the records merged with weights exp2(m_i - max m) and one division.  The emulation passes the family drivers at every (shape,
chunk count) of the GPU file; four mutants each fail at least one:

  neighbour_k_scale   a key scored with the K scale of row r ^ 1
  swapped_scales      the K scale read where the V scale lies and the reverse
  drop_last_block     the last block of every chunk of two or more blocks is never visited
  pad_row_read        rows at and beyond `keys` read as stored (bytes 0x80, NaN scales) instead of as zeros
"""
import ctypes
import os
import re

import numpy as np
import pytest

import attn_cases as ac
import test_attn_prefill_cases_cpu as cases
import test_gpu_attn_prefill_edges as edges
import test_gpu_attn_prefill_i8kv as p8
import test_gpu_attn_rows as rows
import test_gpu_attn_rows_i8kv as r8
from conftest import ROOT

SYMBOL = "eetq_decode_attention_rows_i8kv_f16"
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
CAP = rows.MAX_SPLITS
BLK, WAVES = rows.BLK, 4


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


# ---- the library -------------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_exported(lib):
    from eetq_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eetq_amd.h")).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % SYMBOL, text)
    assert SYMBOL in _lib.EXPORTED_SYMBOLS and hasattr(lib, SYMBOL)
    assert lib.eetq_abi_version() == 7


def test_operator_name():
    import eetq_amd.ops as ops
    assert "decode_attention_rows_i8kv" in ops.__all__
    if ops.BOUNDARY == "ext":
        assert callable(ops.decode_attention_rows_i8kv)
    else:
        assert ops.decode_attention_rows_i8kv is None and ops.decode_attention_rows is None


S_ROWS = 351


def _strides(R=9, H=4, Hkv=2, D=128, S=S_ROWS, **kw):
    st = dict(q_b=R * H * D, q_t=H * D, q_h=D, k_b=Hkv * S * D, k_h=S * D, k_s=D, v_b=Hkv * S * D, v_h=S * D, v_s=D, o_b=R * H * D,
              o_t=H * D, o_h=D)
    st.update(kw)
    return list(st.values())


def _call(lib, q=True, k=True, v=True, sc=True, out=True, ws=True, st=True, sst=True, B=1, H=4, Hkv=2, R=9, keys=340, D=128, splits=2,
          strides=None, scale_strides=None, ws_offset=0, k_offset=0, sc_offset=0, q_offset=0, out_offset=0):
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    at = lambda off: ctypes.c_void_p(base + off)
    arr = (ctypes.c_long * 12)(*(strides or _strides(R=R, H=H, Hkv=Hkv, D=D)))
    sarr = (ctypes.c_long * 3)(*(scale_strides or [Hkv * S_ROWS * 2, S_ROWS * 2, 2]))
    return getattr(lib, SYMBOL)(at(q_offset) if q else None, at(k_offset) if k else None, at(0) if v else None, at(sc_offset) if sc else None,
                                at(out_offset) if out else None, at(ws_offset) if ws else None, B, H, Hkv, R, keys, D, None, 0, splits,
                                ctypes.c_float(0.1), arr if st else None, sarr if sst else None, None)


def test_refusals_without_a_gpu(lib):
    """every refusal returns before any launch: there is no GPU here, and the buffers are 4 KiB of host memory"""
    for missing in ("q", "k", "v", "sc", "out", "st", "sst"):
        assert _call(lib, **{missing: False}) == ERR_INVALID, missing
        assert b"null pointer" in lib.eetq_last_error()
    # the rows / splits / workspace rules of eetq_decode_attention_rows_f16
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
    assert _call(lib, D=256) == ERR_UNSUPPORTED
    assert _call(lib, H=3) == ERR_INVALID                                        # heads not a multiple of kv heads
    # q and out as the fp16 entry
    assert _call(lib, strides=_strides(q_t=4 * 128 + 4)) == ERR_INVALID and b"q strides" in lib.eetq_last_error()
    assert _call(lib, q_offset=8) == ERR_INVALID and b"16-byte aligned" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(o_t=4 * 128 + 2)) == ERR_INVALID and b"out strides" in lib.eetq_last_error()
    assert _call(lib, out_offset=4) == ERR_INVALID and b"out 8-byte" in lib.eetq_last_error()
    # the cache / scale / 2 GiB rules of check_i8_cache, against max_keys
    assert _call(lib, strides=_strides(k_s=132)) == ERR_INVALID and b"8 bytes" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(v_h=351 * 128 + 4)) == ERR_INVALID and b"8 bytes" in lib.eetq_last_error()
    assert _call(lib, k_offset=4) == ERR_INVALID and b"8-byte aligned" in lib.eetq_last_error()
    assert _call(lib, scale_strides=[2 * 351 * 2, 351 * 2, 3]) == ERR_INVALID and b"scale strides" in lib.eetq_last_error()
    assert _call(lib, sc_offset=2) == ERR_INVALID and b"4-byte aligned" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(k_s=1 << 24)) == ERR_INVALID and b"2 GiB" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(v_s=1 << 24)) == ERR_INVALID and b"2 GiB" in lib.eetq_last_error()
    assert _call(lib, scale_strides=[2 * 351 * 2, 351 * 2, 1 << 24]) == ERR_INVALID and b"2 GiB" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(k_s=0)) == ERR_INVALID
    # a row's last bytes must lie inside its own stride (the descriptors end at keys * stride)
    assert _call(lib, strides=_strides(k_s=64)) == ERR_INVALID and b"head_dim bytes" in lib.eetq_last_error()


def test_both_entries_share_their_host_functions(lib):
    """eetq_decode_attention_rows_splits, _max_splits and _workspace_floats serve the int8 entry unchanged: there is no second set"""
    from eetq_amd import _lib
    assert not [n for n in _lib.EXPORTED_SYMBOLS if "rows_i8kv" in n and n != SYMBOL]
    src = open(os.path.join(ROOT, "eetq_amd", "csrc", "attn_decode_rows.hip")).read()
    assert "check_i8_cache(" in src and "int check_i8_cache(" not in src
    assert src.count("void attn_rows_merge_kernel(") == 1, "the merge is reused as it is"


# ---- the promise -------------------------------------------------------------------------------------------------------------

def test_few_rows_int8_promise_is_set_and_restored():
    import eetq_amd.modules.llama_modules as lm
    p = lm._prefill_promise

    def state():
        return tuple(getattr(p, n, False) for n in ("fresh", "appended", "int8_rows", "few_rows", "few_rows_int8"))
    assert state() == (False,) * 5
    with lm.appended_static_prefill(int8_rows=True, few_rows_int8=True):
        assert state() == (False, True, True, False, True)
        with lm.appended_static_prefill(int8_rows=True):
            assert state() == (False, True, True, False, False)
        with lm.appended_static_prefill(few_rows=True):
            assert state() == (False, True, False, True, False)
        assert state() == (False, True, True, False, True)
    assert state() == (False,) * 5
    with pytest.raises(KeyError):
        with lm.appended_static_prefill(int8_rows=True, few_rows_int8=True):
            raise KeyError("x")
    assert state() == (False,) * 5
    with pytest.raises(ValueError, match="int8_rows"):
        with lm.appended_static_prefill(few_rows_int8=True):
            pass
    with pytest.raises(ValueError, match="int8_rows"):
        with lm.appended_static_prefill(few_rows=True, few_rows_int8=True):
            pass
    assert state() == (False,) * 5
    # the fp16 flag on int8 rows keeps its refusal
    with pytest.raises(ValueError, match="fp16 cache rows only"):
        with lm.appended_static_prefill(int8_rows=True, few_rows=True):
            pass
    # under a per-row first key, in either order, as few_rows
    with lm.padded_static_batch(object()):
        with pytest.raises(ValueError, match="padded_static_batch"):
            with lm.appended_static_prefill(int8_rows=True, few_rows_int8=True):
                pass
    with lm.appended_static_prefill(int8_rows=True, few_rows_int8=True):
        with pytest.raises(ValueError, match="few_rows_int8"):
            with lm.padded_static_batch(object()):
                pass
    assert state() == (False,) * 5


def test_graph_decoder_keeps_its_refusal_without_the_opt_in():
    """speculative=k on an int8 cache without kv8_append: refused before the model is looked at"""
    from eetq_amd.utils.graph_decoder import GraphDecoder
    with pytest.raises(ValueError, match="fp16 cache rows"):
        GraphDecoder(None, 1, 32, kv_bits=8, speculative=4)
    with pytest.raises(ValueError, match="kv8_append"):
        GraphDecoder(None, 1, 32, kv_bits=8, speculative=4)


# ---- the emulation -------------------------------------------------------------------------------------------------------------

def _exp2(x):
    return np.exp2(x.astype(np.float64)).astype(np.float32)


def emulate_rows8(q, k8, v8, sc, keys, splits, scale, mutant=None):
    """The int8 few-row kernel's arithmetic on NumPy arrays: q [B, R, H, D] fp16, k8 / v8 int8 [B, Hkv, S, D], sc fp16 [B, Hkv, S, 2]
    -> fp16 [B, R, H, D].  Rows at and beyond `keys` read as bytes 0 and scales 0 (the three descriptors' range)."""
    B, R, H, D = q.shape
    Hkv = k8.shape[1]
    koff = keys - R
    c = np.float32(np.float32(D ** -0.5 if scale is None else scale) * cases.LOG2E)
    hk = np.arange(H) // (H // Hkv)
    nblk = -(-keys // BLK)
    cap = max(nblk, 1) * BLK
    have = min(cap, k8.shape[2]) if mutant == "pad_row_read" else keys
    kint = np.zeros((B, Hkv, cap, D), dtype=np.float32)                       # exact integers
    vint = np.zeros((B, Hkv, cap, D), dtype=np.float16)
    ks = np.zeros((B, Hkv, cap), dtype=np.float32)
    vs = np.zeros((B, Hkv, cap), dtype=np.float16)
    kint[:, :, :have], vint[:, :, :have] = k8[:, :, :have], v8[:, :, :have]
    a, b = (1, 0) if mutant == "swapped_scales" else (0, 1)
    ks[:, :, :have], vs[:, :, :have] = sc[:, :, :have, a], sc[:, :, :have, b]
    if mutant == "neighbour_k_scale":
        ks = ks[:, :, np.arange(cap) ^ 1]
    with np.errstate(invalid="ignore", over="ignore"):
        vv = (vint * vs[..., None]).astype(np.float16).astype(np.float32)     # fp16(vs * v8): ONE rounding of the exact product
        kx = (ks * c).astype(np.float32)                                      # ks * scaling log2 e
        kint, kx, vv = kint[:, hk], kx[:, hk], vv[:, hk]
        qf = q.astype(np.float32).transpose(0, 2, 1, 3)                       # [B, H, R, D]
        lim = np.minimum(keys - 1, koff + np.arange(R))                       # per query row
        recs = []
        for i in range(splits):
            j0, j1 = i * nblk // splits, (i + 1) * nblk // splits
            if mutant == "drop_last_block" and j1 - j0 >= 2:
                j1 -= 1
            waves = []
            for w in range(WAVES):
                m = np.full((B, H, R), -np.inf, dtype=np.float32)
                l = np.zeros((B, H, R), dtype=np.float32)
                o = np.zeros((B, H, R, D), dtype=np.float32)
                for j in range(j0 + w, j1, WAVES):
                    key = j * BLK + np.arange(BLK)
                    s = np.matmul(qf, kint[:, :, key].transpose(0, 1, 3, 2))                       # fp32 q . k8
                    x = (kx[:, :, None, key] * s).astype(np.float32)                              # the K scale, per key, before the mask
                    x = np.where(key[None, :] <= lim[:, None], x, np.float32(-np.inf))            # select
                    mloc = x.max(-1) - cases.P_SHIFT
                    m_new = np.maximum(m, mloc)
                    m_use = np.where(m_new > -np.inf, m_new, np.float32(0))
                    alpha = _exp2(m - m_use)
                    p = _exp2(x - m_use[..., None])
                    l = l * alpha + p.sum(-1, dtype=np.float32)
                    o = o * alpha[..., None] + np.matmul(p.astype(np.float16).astype(np.float32), vv[:, :, key])
                    m = m_new
                waves.append((m, l, o))
            M = np.maximum.reduce([m for m, _, _ in waves])                   # the waves' states -> the chunk's record, in wave order
            M_use = np.where(M > -np.inf, M, np.float32(0))
            L = np.zeros_like(M)
            O = np.zeros((B, H, R, D), dtype=np.float32)
            for m, l, o in waves:
                f = _exp2(m - M_use)
                L, O = L + l * f, O + o * f[..., None]
            recs.append((M, L, O))
        m = np.maximum.reduce([M for M, _, _ in recs])                        # the merge launch
        m_use = np.where(m > -np.inf, m, np.float32(0))
        l = np.zeros_like(m)
        acc = np.zeros((B, H, R, D), dtype=np.float32)
        for M, L, O in recs:
            wgt = _exp2(M - m_use)
            l, acc = l + wgt * L, acc + wgt[..., None] * O
        inv = np.where(l > 0, np.float32(1) / np.where(l > 0, l, np.float32(1)), np.float32(0))
        return (acc * inv[..., None]).astype(np.float16).transpose(0, 2, 1, 3).copy()


def emu_rows8(ns, mutant=None):
    def attend(q, k8, v8, sc, keys, koff, scale):
        assert koff is None
        return emulate_rows8(q, k8, v8, sc, keys, ns, scale, mutant)
    return attend


def _ns(s, n):
    return rows.default_splits(s) if n is None else n


# ---- the conditions the GPU assertions rest on --------------------------------------------------------------------------------

CASES = [(s, D) for s in rows.SHAPES for D in rows.DIMS]
CASE_IDS = [rows._id(s, None, D) for s, D in CASES]


def test_the_gpu_file_runs_the_issue_s_cases():
    assert r8.HOT is rows.HOT and r8.ALL is rows.ALL and r8.CROSS is rows.CROSS and len(rows.SHAPES) == 10
    assert {s.keys for s, n in rows.PAIRS if n is not None} == {130, 340, 528} and rows.FORCED[130] == (1, 2, 3, 64)
    assert [rows._id(s) for s in r8.LAYOUT_SHAPES] == ["B2-R5-H8-2-keys69", "B2-R3-H2-2-keys130"]
    rows.check_chunk_coverage()


@pytest.mark.parametrize("s,D", CASES, ids=CASE_IDS)
def test_inputs_meet_their_preconditions(s, D):
    """the gaps on the DEQUANTISED rows, the pad of bytes 0x80 under NaN scales, a census that notices one row, random cases that build"""
    koff = s.keys - s.T
    if s != rows.SHORT:
        c = p8.staircase_case8(s, D)
        assert c["gap"] >= ac.GAP_MIN and c["gap_scale"] >= ac.GAP_MIN, (c["gap"], c["gap_scale"])
        assert (c["k8"][:, :, s.keys:] == -128).all() and (c["v8"][:, :, s.keys:] == -128).all()
        assert c["k8"].shape[2] == s.keys + ac.PREFILL_PAD and ac.PREFILL_PAD >= 1
        assert np.isnan(c["sc"][:, :, s.keys:]).all() and np.isfinite(c["sc"][:, :, : s.keys].astype(np.float64)).all()
        assert (c["k8"][:, :, : s.keys] != -128).all() and (c["v8"][:, :, : s.keys] != -128).all()
        assert (c["hv"] != 0).any(-1).all(), "a winner's value row is told from the zeros of an unread row"
        for kind in ("diagonal", "permutation"):
            p = p8.pairing_case8(s, D, kind)
            assert p["gap"] >= ac.GAP_MIN, p["gap"]
    cen = p8.census_case8(s, D)
    assert np.array_equal(cen["hv"].astype(np.float64), cen["vd"]) and not cen["q"].any()
    assert (cen["v8"][:, :, s.keys:] == -128).all() and np.isnan(cen["sc"][:, :, s.keys:]).all()
    counts = ac.prefill_counts(s.T, s.keys, koff)
    assert (counts == 0).any() == (s == rows.SHORT)
    drop, dbl = ac.prefix_census_shift_ulps(cen["vd"], counts)
    assert drop > 1.0 and dbl > 1.0, (drop, dbl)
    for scaling, ramp in rows.random_kinds(s):
        r = p8.random_case8(s, D, scaling, ramp)          # raises when no rising ramp exists
        assert (r["k8"][:, :, s.keys:] == -128).all() and np.isnan(r["sc"][:, :, s.keys:]).all()
        b = p8.bound8(r["ref"], r["absmean"])
        assert (np.abs(r["ref"].astype(np.float16).astype(np.float64) - r["ref"]) <= b).all()
    assert (s == rows.NO_RAMP) == (len(rows.random_kinds(s)) == 2)


# ---- the emulation passes every family, every mutant fails one ---------------------------------------------------------------------

HOT_PAIRS = [(s, n, D) for s, n, D in rows.HOT]
ALL_PAIRS = [(s, n, D) for s, n, D in rows.ALL]


@pytest.mark.parametrize("s,n,D", HOT_PAIRS, ids=rows._ids(HOT_PAIRS))
def test_emulation_passes_the_exact_families(s, n, D):
    ns = _ns(s, n)
    r8.drive_edge_rows8(emu_rows8(ns), s, D, ns)
    r8.drive_by_scale_rows8(emu_rows8(ns), s, D, ns)
    p8.drive_pairing8(emu_rows8(ns), s, D, "diagonal")
    p8.drive_pairing8(emu_rows8(ns), s, D, "permutation")


@pytest.mark.parametrize("s,n,D", ALL_PAIRS, ids=rows._ids(ALL_PAIRS))
def test_emulation_passes_census_and_random(s, n, D):
    ns = _ns(s, n)
    ulp = p8.drive_census8(emu_rows8(ns), s, D)
    ratios = [p8.drive_random8(emu_rows8(ns), s, D, scl, ramp) for scl, ramp in rows.random_kinds(s)]
    print("attn-rows-i8kv emulation %s: census %.4f ulp, random ratios %s" % (rows._id(s, n, D), ulp, ["%.3f" % r for r in ratios]))


S130, S340, S69 = rows.SHAPES[4], rows.SHAPES[5], rows.SHAPES[2]
assert (S130.keys, S340.keys, S69.keys) == (130, 340, 69)


def _edge(attend, s, D, ns):
    r8.drive_edge_rows8(attend, s, D, ns)


def _by_scale(attend, s, D, ns):
    r8.drive_by_scale_rows8(attend, s, D, ns)


def _census(attend, s, D, ns):
    p8.drive_census8(attend, s, D)


def _random(attend, s, D, ns):
    p8.drive_random8(attend, s, D, "default", False)


def _diagonal(attend, s, D, ns):
    p8.drive_pairing8(attend, s, D, "diagonal")


MUTANTS = {
    # name: [(driver, shape, chunk count)] -- every listed run must fail, at both head sizes
    "neighbour_k_scale": [(_by_scale, S130, 2), (_by_scale, S340, 3)],
    "swapped_scales": [(_edge, S130, 2), (_census, S340, 3), (_diagonal, S69, 1), (_random, S130, 1)],
    "drop_last_block": [(_census, S340, 3), (_census, S130, 2), (_edge, S340, 3), (_diagonal, S340, 2)],
    "pad_row_read": [(_census, S130, 2), (_random, S340, 3), (_edge, S69, 1)],
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
@pytest.mark.parametrize("D", edges.DIMS)
def test_mutant_is_caught(name, D):
    for fn, s, ns in MUTANTS[name]:
        assert cases._fails(fn, emu_rows8(ns, name), s, D, ns), "%s passes %s on %s at %d chunks, D = %d" % (name, fn.__name__, s, ns, D)
        fn(emu_rows8(ns), s, D, ns)   # and the unmutated emulation passes the same run
