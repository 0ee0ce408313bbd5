"""Prompt attention behind int8 cache rows without a GPU: the new C-ABI entry (declared, exported, ABI still 7, refusing bad
arguments before any launch), the third prompt promise of llama_modules, and a NumPy emulation of the NEW arithmetic -- K bytes as
exact integers in the first product, the K scale folded into the fp32 score behind it, V rows staged as fp16(vs * v8), otherwise
the steps of tests/test_attn_prefill_cases_cpu.py::emulate -- that goes through the family drivers of
tests/test_gpu_attn_prefill_i8kv.py at its shapes and passes them, while three mutants each fail at least one family:

  neighbour_k_scale   a key read with the K scale of row r ^ 1
  group_v_scale       the V rows of a staged group given each other's scale (row r takes the V scale of r ^ 1)
  unsigned_bytes      cache bytes read as unsigned

The inputs' preconditions are proved here: the 200-unit gaps AFTER quantisation (hot over random, hotter over hot, the hot row
over its decoys, every pairing), the census's sensitivity to one dropped or doubled row and to a V scale shifted by one row, and
that the reference arithmetic (float64 on the dequantised rows, then rounded to fp16) stays inside the random bound."""
import ctypes
import os
import re

import numpy as np
import pytest

import attn_cases as ac
import kv8_cases as k8c
import test_attn_prefill_cases_cpu as cases
import test_gpu_attn_prefill_append as app
import test_gpu_attn_prefill_edges as edges
import test_gpu_attn_prefill_i8kv as i8
from conftest import ROOT

SYMBOL = "eetq_prefill_attention_i8kv_f16"
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
TABLE = [(r, i, D) for r in i8.TABLE_ROWS if r != 7 for i in range(len(edges.ROWS[r])) for D in edges.DIMS]
TABLE_IDS = ["row%d.%d-D%d" % t for t in TABLE]
SPLIT_SHAPES = sorted(set(s for s, _ in app.SPLIT))
SPLIT_TABLE = [(i, D) for i in range(len(SPLIT_SHAPES)) for D in edges.DIMS]
SPLIT_TABLE_IDS = ["T%d-keys%d-D%d" % (SPLIT_SHAPES[i].T, SPLIT_SHAPES[i].keys, D) for i, D in SPLIT_TABLE]


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


def test_bindings_expose_the_op():
    import eetq_amd.ops as ops
    assert hasattr(ops, "prefill_attention_i8kv")
    if ops.BOUNDARY == "ctypes":
        assert ops.prefill_attention_i8kv is None and ops.prefill_attention is None
    else:
        assert callable(ops.prefill_attention_i8kv)


def _call(lib, q=True, k=True, v=True, sc=True, out=True, ws=True, st=True, sst=True, B=1, H=4, Hkv=2, T=40, keys=340, D=128, splits=2,
          strides=None, scale_strides=None, ws_offset=0, k_offset=0, sc_offset=0, q_offset=0):
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    S = 351
    arr = (ctypes.c_long * 12)(*(strides or [T * H * D, H * D, D, Hkv * S * D, S * D, D, Hkv * S * D, S * D, D, T * H * D, H * D, D]))
    sarr = (ctypes.c_long * 3)(*(scale_strides or [Hkv * S * 2, S * 2, 2]))
    return getattr(lib, SYMBOL)(ctypes.c_void_p(base + q_offset) if q else None, ctypes.c_void_p(base + k_offset) if k else None,
                                p if v else None, ctypes.c_void_p(base + sc_offset) if sc else None, p if out else None,
                                ctypes.c_void_p(base + ws_offset) if ws else None, B, H, Hkv, T, keys, D, None, 0, splits,
                                ctypes.c_float(0.1), arr if st else None, sarr if sst else None, None)


def _strides(T=40, H=4, Hkv=2, D=128, S=351, **kw):
    st = dict(q_b=T * H * D, q_t=H * D, q_h=D, k_b=Hkv * S * D, k_h=S * D, k_s=D, v_b=Hkv * S * D, v_h=S * D, v_s=D, o_b=T * H * D,
              o_t=H * D, o_h=D)
    st.update(kw)
    return list(st.values())


def test_refusals_without_a_gpu(lib):
    """Every EETQ_ERR_INVALID / EETQ_ERR_UNSUPPORTED case returns before any launch (there is no device here to launch on)."""
    for missing in ("q", "k", "v", "sc", "out", "st", "sst"):
        assert _call(lib, **{missing: False}) == ERR_INVALID, missing
        assert b"null pointer" in lib.eetq_last_error()
    assert _call(lib, splits=0) == ERR_INVALID and b"splits" in lib.eetq_last_error()
    assert _call(lib, splits=17) == ERR_INVALID and b"splits" in lib.eetq_last_error()
    assert _call(lib, ws=False) == ERR_INVALID and b"workspace" in lib.eetq_last_error()
    assert _call(lib, ws_offset=4) == ERR_INVALID and b"workspace" in lib.eetq_last_error()
    assert _call(lib, keys=0) == ERR_INVALID and b"max_keys" in lib.eetq_last_error()
    assert _call(lib, keys=-5, splits=1, ws=False) == ERR_INVALID
    assert _call(lib, D=96) == ERR_UNSUPPORTED
    assert _call(lib, D=256) == ERR_UNSUPPORTED
    assert _call(lib, H=3) == ERR_INVALID
    # the rules of eetq_decode_attention_i8kv_f16: 8-byte cache strides and alignment, dword scale pairs, the 2 GiB range
    assert _call(lib, strides=_strides(k_s=132)) == ERR_INVALID and b"8 bytes" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(v_h=351 * 128 + 4)) == ERR_INVALID and b"8 bytes" in lib.eetq_last_error()
    assert _call(lib, k_offset=4) == ERR_INVALID and b"8-byte aligned" in lib.eetq_last_error()
    assert _call(lib, scale_strides=[2 * 351 * 2, 351 * 2, 3]) == ERR_INVALID and b"scale strides" in lib.eetq_last_error()
    assert _call(lib, sc_offset=2) == ERR_INVALID and b"4-byte aligned" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(k_s=1 << 24)) == ERR_INVALID and b"2 GiB" in lib.eetq_last_error()
    assert _call(lib, scale_strides=[2 * 351 * 2, 351 * 2, 1 << 24]) == ERR_INVALID and b"2 GiB" in lib.eetq_last_error()
    # q as the fp16 prompt entry: strides of 8 elements, 16-byte alignment
    assert _call(lib, strides=_strides(q_t=4 * 128 + 4)) == ERR_INVALID and b"q strides" in lib.eetq_last_error()
    assert _call(lib, q_offset=8) == ERR_INVALID and b"16-byte aligned" in lib.eetq_last_error()
    assert _call(lib, strides=_strides(o_t=4 * 128 + 2)) == ERR_INVALID and b"out strides" in lib.eetq_last_error()


def test_a_cache_the_decode_entry_accepts_is_accepted():
    """The shared rule (kv_i8.hpp::check_i8_cache) is one function: both entries call it with the cache's six strides."""
    src = open(os.path.join(ROOT, "eetq_amd", "csrc", "attn_prefill.hip")).read()
    dec = open(os.path.join(ROOT, "eetq_amd", "csrc", "attn_decode.hip")).read()
    hdr = open(os.path.join(ROOT, "eetq_amd", "csrc", "kv_i8.hpp")).read()
    assert hdr.count("int check_i8_cache(") == 1 and "check_i8_cache(" in src and "check_i8_cache(" in dec
    assert "int check_i8_cache(" not in src and "int check_i8_cache(" not in dec


# ---- the promise -------------------------------------------------------------------------------------------------------------

def test_int8_rows_promise_is_set_and_restored():
    import eetq_amd.modules.llama_modules as lm
    p = lm._prefill_promise

    def state():
        return getattr(p, "fresh", False), getattr(p, "appended", False), getattr(p, "int8_rows", False)
    assert state() == (False, False, False)
    with lm.appended_static_prefill():
        assert state() == (False, True, False)
    with lm.appended_static_prefill(int8_rows=True):
        assert state() == (False, True, True)
        with lm.appended_static_prefill():                       # the plain promise inside: int8 rows are NOT accepted there
            assert state() == (False, True, False)
        assert state() == (False, True, True)
        with lm.fresh_static_prefill():
            assert state() == (True, True, True)
        assert state() == (False, True, True)
    assert state() == (False, False, False)
    with lm.fresh_static_prefill():
        with lm.appended_static_prefill(int8_rows=True):
            assert state() == (False, True, True)
        assert state() == (True, False, False)
    with pytest.raises(KeyError):
        with lm.appended_static_prefill(int8_rows=True):
            raise KeyError("x")
    assert state() == (False, False, False)


def test_graph_decoder_refuses_the_switch_on_an_fp16_cache():
    from eetq_amd.utils.graph_decoder import GraphDecoder
    with pytest.raises(ValueError, match="kv8_append"):
        GraphDecoder(None, 1, 8, kv_bits=16, kv8_append=True)


# ---- the emulation -------------------------------------------------------------------------------------------------------------

def emulate8(q, k8, v8, sc, keys, koff, scale, mutant=None):
    """The int8-row kernel's arithmetic on NumPy arrays: q [B, T, H, D] fp16, k8, v8 int8 [B, Hkv, S, D], sc fp16 [B, Hkv, S, 2]
    -> fp16 [B, T, H, D].  Rows at and beyond `keys` read as bytes 0 and scale 0 (the three descriptors' range)."""
    B, T, H, D = q.shape
    Hkv = k8.shape[1]
    koff = keys - T if koff is None else koff
    c = np.float32(np.float32(D ** -0.5 if scale is None else scale) * cases.LOG2E)
    hk = np.arange(H) // (H // Hkv)
    nb_all = -(-keys // 64)
    rows = max(nb_all, 1) * 64
    if mutant == "unsigned_bytes":
        k8, v8 = k8.view(np.uint8), v8.view(np.uint8)
    kint = np.zeros((B, Hkv, rows, D), dtype=np.float32)                      # exact integers (fp16 holds them, so does fp32)
    ks = np.zeros((B, Hkv, rows), dtype=np.float32)
    vs = np.zeros((B, Hkv, rows), dtype=np.float16)
    vint = np.zeros((B, Hkv, rows, D), dtype=np.float16)
    kint[:, :, :keys], vint[:, :, :keys] = k8[:, :, :keys], v8[:, :, :keys]
    ks[:, :, :keys], vs[:, :, :keys] = sc[:, :, :keys, 0], sc[:, :, :keys, 1]
    r = np.arange(rows)
    if mutant == "neighbour_k_scale":
        ks = ks[:, :, r ^ 1]
    if mutant == "group_v_scale":
        vs = vs[:, :, r ^ 1]
    vv = (vint * vs[..., None]).astype(np.float16).astype(np.float32)         # fp16(vs * v8): ONE rounding of the exact product
    kint, ks, vv = kint[:, hk], ks[:, hk], vv[:, hk]
    qf = q.astype(np.float32).transpose(0, 2, 1, 3)
    t = np.arange(T)
    q0, w0 = (t // 128) * 128, (t // 32) * 32
    kend = np.minimum(keys, q0 + 128 + koff)
    nblk = np.where(kend > 0, -(-kend // 64), 0)
    m = np.full((B, H, T), -np.inf, dtype=np.float32)
    l = np.zeros((B, H, T), dtype=np.float32)
    o = np.zeros((B, H, T, D), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(nb_all):
            key0 = j * 64
            key = key0 + np.arange(64)
            run = (j < nblk) & (key0 <= w0 + 31 + koff)
            if not run.any():
                continue
            edge = (key0 + 63 > w0 + koff) | (key0 + 64 > keys)
            valid = (key[None, :] <= (t + koff)[:, None]) & (key[None, :] < keys)
            masked = edge[:, None] & ~valid
            s = np.matmul(qf, kint[:, :, key0: key0 + 64].transpose(0, 1, 3, 2))          # fp32 q . k8
            s = (s * ks[:, :, None, key0: key0 + 64]).astype(np.float32)                  # the K scale, in fp32, before the mask
            s = np.where(masked, np.float32(-np.inf), s)
            mloc = (s.max(-1).astype(np.float64) * np.float64(c) - np.float64(cases.P_SHIFT)).astype(np.float32)
            m_new = np.maximum(m, mloc)
            m_use = np.where(m_new > -np.inf, m_new, np.float32(0))
            alpha = np.exp2((m - m_use).astype(np.float64)).astype(np.float32)
            p = np.exp2(s.astype(np.float64) * np.float64(c) - m_use[..., None].astype(np.float64)).astype(np.float32)
            p = np.where(np.isnan(p), np.float32(0), p)
            l_new = l * alpha + p.sum(-1, dtype=np.float32)
            o_new = o * alpha[..., None] + np.matmul(p.astype(np.float16).astype(np.float32), vv[:, :, key0: key0 + 64])
            m, l, o = np.where(run, m_new, m), np.where(run, l_new, l), np.where(run[:, None], o_new, o)
        inv = np.where(l > 0, np.float32(1) / np.where(l > 0, l, np.float32(1)), np.float32(0))
        return (o * inv[..., None]).astype(np.float16).transpose(0, 2, 1, 3).copy()


def emu8(mutant=None):
    return lambda q, k8, v8, sc, keys, koff, scale: emulate8(q, k8, v8, sc, keys, koff, scale, mutant)


def _shape(row, i):
    return edges.ROWS[row][i]


# ---- the conditions the GPU assertions rest on --------------------------------------------------------------------------------

def _all_shapes():
    return [(_shape(r, i), D) for r, i, D in TABLE] + [(SPLIT_SHAPES[i], D) for i, D in SPLIT_TABLE]


def test_gaps_hold_after_quantisation():
    """hot over every random row, hotter over hot, the hot row over its eighth-scale decoys: >= 200 on the DEQUANTISED rows;
    the pad rows are bytes 0x80 under NaN scales, and no valid row holds a byte 0x80."""
    for s, D in _all_shapes():
        c = i8.staircase_case8(s, D)
        assert c["gap"] >= ac.GAP_MIN and c["gap_scale"] >= ac.GAP_MIN, (s, D, c["gap"], c["gap_scale"])
        assert (c["k8"][:, :, s.keys:] == -128).all() and (c["v8"][:, :, s.keys:] == -128).all() and c["k8"].shape[2] == s.keys + i8.PAD
        assert np.isnan(c["sc"][:, :, s.keys:]).all() and np.isfinite(c["sc"][:, :, : s.keys].astype(np.float64)).all()
        assert (c["k8"][:, :, : s.keys] != -128).all() and (c["v8"][:, :, : s.keys] != -128).all()


PAIRED = [(r, i, D, kind) for r, i, D in TABLE for kind in ("diagonal", "permutation") if r in (1, 2, 3, 4)]


@pytest.mark.parametrize("row,i,D,kind", PAIRED, ids=["row%d.%d-D%d-%s" % p for p in PAIRED])
def test_pairing_gap_is_200_after_quantisation(row, i, D, kind):
    s = _shape(row, i)
    c = i8.pairing_case8(s, D, kind)
    assert c["gap"] >= ac.GAP_MIN, c["gap"]
    ref, _ = ac.prefill_reference(c["q"], c["kd"], c["vd"], s.keys, edges.koff_of(s), c["scale"])
    ref16 = ref.astype(np.float16)
    ref16[ref16 == 0] = 0          # a byte 0 gives +0; the float64 tail of the other rows may leave -0 here
    assert not ac.check_pairing(ref16, dict(pi=c["pi"], v=c["hv"])).any()


@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_census_sees_a_row_and_a_shifted_v_scale(row, i, D):
    """One dropped or doubled row moves the mean by more than 3 fp16 ulp at every prefix length, and so does reading every V
    row with its neighbour's scale; vs * v8 is exact in fp16."""
    s = _shape(row, i)
    c = i8.census_case8(s, D)
    assert np.array_equal(c["hv"].astype(np.float64), c["vd"]) and not c["q"].any()
    counts = ac.prefill_counts(s.T, s.keys, edges.koff_of(s))
    if not counts.any():
        return
    drop, dbl = ac.prefix_census_shift_ulps(c["vd"], counts)
    assert drop > 3.0 and dbl > 3.0, (drop, dbl)
    vs = c["sc"][:, :, : s.keys, 1]
    shifted = k8c.dequantize_rows(c["v8"][:, :, : s.keys], vs[:, :, np.minimum(np.arange(s.keys) ^ 1, s.keys - 1)])
    ref2, _ = ac.prefill_reference(c["q"], c["kd"], shifted, s.keys, edges.koff_of(s), c["scale"])
    seen = counts > 1
    moved = (np.abs(ref2 - c["ref"]) / ac.fp16_ulp(c["ref"])).max(-1)[:, seen]
    assert moved.max() > 3.0


@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_reference_arithmetic_stays_inside_the_random_bound(row, i, D):
    """The float64 reference rounded to fp16 is within bound8 of itself (half an ulp), and a reference whose V rows are rounded
    to fp16 first -- the one step the int8 form adds -- stays within the ADDED term alone."""
    s = _shape(row, i)
    for scaling, ramp in edges.RANDOM_KINDS:
        c = i8.random_case8(s, D, scaling, ramp)
        b = i8.bound8(c["ref"], c["absmean"])
        assert (np.abs(c["ref"].astype(np.float16).astype(np.float64) - c["ref"]) <= b).all()
        rounded, _ = ac.prefill_reference(c["q"], c["kd"], c["hv"].astype(np.float64), s.keys, edges.koff_of(s), c["scale"])
        assert (np.abs(rounded - c["ref"]) <= 2.0 ** -11 * c["absmean"] + 2.0 ** -25).all()


# ---- the emulation passes every family ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_emulation_passes_the_exact_families_and_the_census(row, i, D):
    s = _shape(row, i)
    if row in (1, 2, 3, 5):
        i8.drive_staircase8(emu8(), s, D)
        i8.drive_by_scale8(emu8(), s, D)
    if row in (1, 2, 3, 4):
        i8.drive_pairing8(emu8(), s, D, "diagonal")
        i8.drive_pairing8(emu8(), s, D, "permutation")
    ulp = i8.drive_census8(emu8(), s, D)
    print("prefill-i8kv emulation row %d.%d D=%d: census %.4f ulp" % (row, i, D, ulp))


@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_emulation_stays_within_the_random_bound(row, i, D):
    s = _shape(row, i)
    ratios = [i8.drive_random8(emu8(), s, D, scaling, ramp) for scaling, ramp in edges.RANDOM_KINDS]
    print("prefill-i8kv emulation row %d.%d D=%d: random ratios %s" % (row, i, D, ["%.3f" % r for r in ratios]))


@pytest.mark.parametrize("i,D", SPLIT_TABLE, ids=SPLIT_TABLE_IDS)
def test_emulation_passes_the_families_at_the_split_shapes(i, D):
    """The split shapes through the unsplit arithmetic (the shares and the merge are the fp16 form's, emulated in
    tests/test_attn_prefill_append_cpu.py)."""
    s = SPLIT_SHAPES[i]
    i8.drive_staircase8(emu8(), s, D)
    i8.drive_by_scale8(emu8(), s, D)
    if s.koff is None:
        i8.drive_pairing8(emu8(), s, D, "diagonal")
        i8.drive_pairing8(emu8(), s, D, "permutation")
    i8.drive_census8(emu8(), s, D)
    for scaling, ramp in edges.RANDOM_KINDS:
        i8.drive_random8(emu8(), s, D, scaling, ramp)


# ---- every mutant fails some family ----------------------------------------------------------------------------------------------

ROW1, ROW2 = edges.ROWS[1][0], edges.ROWS[2][0]

MUTANTS = {
    "neighbour_k_scale": [(i8.drive_by_scale8, ROW1, ()), (i8.drive_by_scale8, ROW2, ())],
    "group_v_scale": [(i8.drive_census8, ROW1, ()), (i8.drive_census8, ROW2, ()), (i8.drive_staircase8, ROW1, ()),
                      (i8.drive_pairing8, ROW2, ("permutation",))],
    "unsigned_bytes": [(i8.drive_staircase8, ROW1, ()), (i8.drive_census8, ROW2, ()), (i8.drive_pairing8, ROW1, ("diagonal",)),
                       (i8.drive_random8, ROW2, ("default", False))],
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
@pytest.mark.parametrize("D", edges.DIMS)
def test_mutant_is_caught(name, D):
    for fn, s, extra in MUTANTS[name]:
        assert cases._fails(fn, emu8(name), s, D, *extra), "%s passes %s on %s at D = %d" % (name, fn.__name__, s, D)
