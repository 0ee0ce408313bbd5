"""Few-row attention behind INT8 cache rows (``ops.decode_attention_rows_i8kv``, eetq_decode_attention_rows_i8kv_f16: the KV8
instantiations of eetq_amd/csrc/attn_decode_rows.hip) at D = 128 and D = 64, at the shapes, chunk counts, hot rows and two-step pairs
of tests/test_gpu_attn_rows.py, on the int8 cases and through the family drivers of tests/test_gpu_attn_prefill_i8kv.py.  The
references are attn_cases.prefill_reference in float64 on kv8_cases.dequantize_rows, and kv8_cases.hot_value; they share no code with
the kernel.

  staircase    the QUANTISED hot key (bytes and K scale together) at rows.hot_rows -- row 0, the last row, around every 32-key edge
               and every chunk boundary, the whole causal tail -- and at rows.two_step_pairs: out[t] == fp16(vs v8) of the winner
               BIT FOR BIT, bait rows within bound8
  by K scale   the same rows; rows r - 1 and r + 1 carry the hot bytes with an eighth of the K scale
  pairing      diagonal and permutation, bit for bit
  census       within 1 fp16 ulp of the float64 mean; rows with nothing to attend give zeros (the keys < R shape included)
  random       |out - ref| <= bound8(ref, absmean) = attn_cases.random_bound + one fp16 rounding of every vs v8
  layouts, device length (bit for bit against the host-length call of the same entry), the cross-check against
  ops.prefill_attention_i8kv (|rows - prompt| <= 2 bound8: one contract, two tilings), argument checks

Every cache carries PREFILL_PAD rows of bytes 0x80 and NaN scales behind ``keys``; ``kv_len`` is on the device.  Every call runs on a
NaN-filled workspace, a zero-filled one and a NaN-filled one again and must give the same bits; no output may be NaN.
tests/test_attn_rows_i8kv_cpu.py builds every case here on the CPU and runs the drivers on a NumPy emulation and its mutants.

290 cases, 6.0 s wall for the file on an MI355X; every family passed as the kernel was first written.  Largest figures over all
shapes and chunk counts, D = 128 / D = 64:

  random: |out - ref| / bound8                                      0.476 / 0.467
  census: error in fp16 ulp                                         0.4990 / 0.4995
  staircase bait rows: |out - ref| / bound8                         0.356 / 0.356
  cross-check: |rows - prompt| / (2 bound8)                         0.199 / 0.288
"""
import numpy as np
import pytest
import torch

import attn_cases as ac
import test_gpu_attn_prefill_edges as edges
import test_gpu_attn_prefill_i8kv as p8
import test_gpu_attn_rows as rows_t
from test_gpu_attn_rows import FORCED, SHAPES, SHORT, Shape, _id, default_splits, hot_rows, random_kinds, two_step_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = edges.DIMS
MAX_SPLITS = rows_t.MAX_SPLITS
assert FORCED == {130: (1, 2, 3, 64), 340: (1, 2, 3, 64), 528: (1, 2, 3, 64)}


# ---- this file's drivers: the int8 steps of p8 at the rows of rows_t; attend(q, k8, v8, sc, keys, koff, scale) ------------------

def drive_edge_rows8(attend, s, D, ns):
    c = p8.staircase_case8(s, D)
    assert c["gap"] >= ac.GAP_MIN, c["gap"]
    heads, worst = s.B * s.Hkv, 0.0
    hot, hotter = (c["hot8"], c["hots"], 1), (c["hotter8"], c["hotters"], 2)
    rows = hot_rows(s, ns)
    for i in range(0, len(rows), heads):
        r = np.resize(np.array(rows[i: i + heads]), heads).reshape(s.B, s.Hkv)
        bad, ratio = p8._steps_launch8(attend, s, c, [(r,) + hot])
        worst = max(worst, ratio)
        assert not bad.any(), "hot rows %s: %s" % (r.reshape(-1).tolist(), edges._first(bad, "query rows"))
    pairs = two_step_pairs(s, ns)
    for i in range(0, len(pairs), heads):
        pr = np.resize(np.array(pairs[i: i + heads]), (heads, 2))
        r1, r2 = pr[:, 0].reshape(s.B, s.Hkv), pr[:, 1].reshape(s.B, s.Hkv)
        for first, second, name in ((hot, hotter, "hot then hotter"), (hotter, hot, "hotter then hot")):
            bad, ratio = p8._steps_launch8(attend, s, c, [(r1,) + first, (r2,) + second])
            worst = max(worst, ratio)
            assert not bad.any(), "%s at %s: %s" % (name, pr.tolist(), edges._first(bad, "query rows"))
    return worst


def drive_by_scale_rows8(attend, s, D, ns):
    """p8.drive_by_scale8 at rows_t.hot_rows: rows r - 1 and r + 1 carry the hotter key's bytes with an eighth of its K scale; every
    query that sees row r returns fp16(vs[r] v8[r]) bit for bit"""
    c = p8.staircase_case8(s, D)
    assert c["gap_scale"] >= ac.GAP_MIN, c["gap_scale"]
    heads = s.B * s.Hkv
    rows = [r for r in hot_rows(s, ns) if 1 <= r <= s.keys - 2]
    for i in range(0, len(rows), heads):
        r = np.resize(np.array(rows[i: i + heads]), heads).reshape(s.B, s.Hkv)
        k8, sc = p8.place(c, [(r - 1, c["hotter8"], c["eighth"]), (r + 1, c["hotter8"], c["eighth"]), (r, c["hotter8"], c["hotters"])])
        out = attend(c["q"], k8, c["v8"], sc, s.keys, s.koff, None)
        assert not np.isnan(out).any(), "NaN in the output"
        win = ac.staircase_winner(s.T, edges.koff_of(s), [(r, 1)])
        B, T, H, _ = out.shape
        w = ac.expand_heads(win, H).transpose(0, 2, 1)
        exp = ac.expand_heads(c["hv"], H)[np.arange(B)[:, None, None], np.arange(H)[None, None, :], np.maximum(w, 0)]
        bad = (w >= 0) & ac.bits_differ(out, exp)
        assert not bad.any(), "hot by scale at rows %s: %s" % (r.reshape(-1).tolist(), edges._first(bad, "query rows"))
    p8.drive_by_scale8(attend, s, D)   # and at the prompt file's own edge rows


# ---- the GPU side ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.BOUNDARY != "ext":
        pytest.skip("decode_attention_rows_i8kv lives in the compiled module")
    assert o.decode_attention_rows_i8kv is not None and o.prefill_attention_i8kv is not None   # missing there: a failure
    return o


_len, _same_bits = rows_t._len, rows_t._same_bits


def _dev(c, layout="plain"):
    return (edges._lay_q(c["q"], "fusedq" if layout == "bshd" else layout), p8._lay_cache(c["k8"], layout), p8._lay_cache(c["v8"], layout),
            p8._lay_scales(c["sc"], layout))


def rows_attend8(ops, splits=None, layout="plain"):
    """attend of the family drivers: max_keys = the whole cache (the 0x80 / NaN rows included), kv_len on the device, koff = None.
    Three calls -- a NaN-filled, a zero-filled, a NaN-filled workspace -- with equal bits."""
    def attend(q, k8, v8, sc, keys, koff, scale):
        assert koff is None
        kw = {} if scale is None else {"scaling": scale}
        qd, kd, vd, sd = _dev(dict(q=q, k8=k8, v8=v8, sc=sc), layout)
        cap = kd.shape[2]
        assert cap == keys + ac.PREFILL_PAD
        n = rows_t.ws_floats(ops, q, cap, k8.shape[1], splits)
        outs = []
        for fill in (float("nan"), 0.0, float("nan")):
            ws = torch.full((n,), fill, dtype=torch.float32, device=DEV)
            outs.append(ops.decode_attention_rows_i8kv(qd, kd, vd, sd, cap, kv_len=_len(keys), splits=splits, workspace=ws, **kw))
        assert _same_bits(outs[0], outs[1]), "the result depends on what the workspace held"
        assert _same_bits(outs[0], outs[2]), "a repeated call gives other bits"
        assert outs[0].shape == q.shape and outs[0].is_contiguous() and outs[0].dtype == torch.float16
        return outs[0].cpu().numpy()
    return attend


HOT, ALL = rows_t.HOT, rows_t.ALL
_ids = rows_t._ids


def test_the_cases_are_the_issue_s():
    assert len(SHAPES) == 10 and len(ALL) == 2 * (10 + 3 * 4) and SHORT in SHAPES and (SHORT, None, 128) not in HOT
    rows_t.check_chunk_coverage()


@pytest.mark.parametrize("s,n,D", HOT, ids=_ids(HOT))
def test_staircase_edge_rows_and_two_steps(ops, s, n, D):
    ns = default_splits(s) if n is None else n
    worst = drive_edge_rows8(rows_attend8(ops, n), s, D, ns)
    print("attn-rows-i8kv staircase-bait edges %s: max ratio %.3f" % (_id(s, n, D), worst))


@pytest.mark.parametrize("s,n,D", HOT, ids=_ids(HOT))
def test_hot_by_k_scale_alone(ops, s, n, D):
    drive_by_scale_rows8(rows_attend8(ops, n), s, D, default_splits(s) if n is None else n)


@pytest.mark.parametrize("kind", ("diagonal", "permutation"))
@pytest.mark.parametrize("s,n,D", HOT, ids=_ids(HOT))
def test_pairing(ops, s, n, D, kind):
    p8.drive_pairing8(rows_attend8(ops, n), s, D, kind)


@pytest.mark.parametrize("s,n,D", ALL, ids=_ids(ALL))
def test_prefix_census(ops, s, n, D):
    worst = p8.drive_census8(rows_attend8(ops, n), s, D)
    print("attn-rows-i8kv census %s: max error %.4f ulp" % (_id(s, n, D), worst))


@pytest.mark.parametrize("s,n,D", ALL, ids=_ids(ALL))
def test_random(ops, s, n, D):
    worst = max(p8.drive_random8(rows_attend8(ops, n), s, D, sc, ramp) for sc, ramp in random_kinds(s))
    print("attn-rows-i8kv random %s: max ratio %.4f" % (_id(s, n, D), worst))


LAYOUT_SHAPES = [Shape(2, 5, 8, 2, 69, None), Shape(2, 3, 2, 2, 130, None)]
assert [_id(s) for s in LAYOUT_SHAPES] == ["B2-R5-H8-2-keys69", "B2-R3-H2-2-keys130"]


@pytest.mark.parametrize("s", LAYOUT_SHAPES, ids=[_id(s) for s in LAYOUT_SHAPES])
@pytest.mark.parametrize("D", DIMS)
def test_layouts(ops, s, D):
    """[B, S, Hkv, D] byte storage, scale pairs strided inside wider storage, the query a view of a fused QKV row"""
    attend = rows_attend8(ops, None, "bshd")
    ns = default_splits(s)
    drive_edge_rows8(attend, s, D, ns)
    drive_by_scale_rows8(attend, s, D, ns)
    p8.drive_pairing8(attend, s, D, "diagonal")
    p8.drive_census8(attend, s, D)
    p8.drive_random8(attend, s, D, "default", False)


@pytest.mark.parametrize("layout", ("plain", "bshd"))
@pytest.mark.parametrize("s", rows_t.DEVLEN, ids=[_id(s) for s in rows_t.DEVLEN])
@pytest.mark.parametrize("D", DIMS)
def test_device_length(ops, s, D, layout):
    """The cases of test_gpu_attn_rows.test_device_length -- exact, shorter, biased, clamped beyond max_keys, 0 and negative (zeros) --
    against the host-length call of the SAME entry with max_keys = the effective keys, bit for bit, at 1 and 3 chunks."""
    c = p8.random_case8(s, D, "default", True)
    q, k8, v8, sc = _dev(c, layout)
    cap = k8.shape[2]
    assert cap == s.keys + ac.PREFILL_PAD
    for ns in (1, 3):
        for n, bias, mk, eff in ((s.keys, 0, cap, s.keys), (s.keys - 40, 0, cap, s.keys - 40), (s.keys - 7, 5, cap, s.keys - 2),
                                 (s.keys + 3, -20, cap, s.keys - 17), (s.keys + 1000, 0, s.keys, s.keys), (cap, 2, s.keys - 1, s.keys - 1),
                                 (5, 0, cap, 5)):
            host = ops.decode_attention_rows_i8kv(q, k8, v8, sc, eff, splits=ns)
            dev = ops.decode_attention_rows_i8kv(q, k8, v8, sc, mk, kv_len=_len(n), kv_len_bias=bias, splits=ns)
            assert not torch.isnan(dev).any()
            assert _same_bits(host, dev), (ns, n, bias, mk)
        zero = ops.decode_attention_rows_i8kv(q, k8, v8, sc, cap, kv_len=_len(0), splits=ns)
        below = ops.decode_attention_rows_i8kv(q, k8, v8, sc, cap, kv_len=_len(9), kv_len_bias=-12, splits=ns)
        assert not zero.any() and not below.any() and not torch.isnan(zero).any() and not torch.isnan(below).any()


CROSS = rows_t.CROSS


@pytest.mark.parametrize("s,n,D", CROSS, ids=_ids(CROSS))
def test_cross_check_against_the_prompt_kernel(ops, s, n, D):
    """|rows - prompt| <= 2 bound8: both calls implement one contract on different tiles (not bit equality)"""
    worst = 0.0
    for scl, ramp in random_kinds(s):
        c = p8.random_case8(s, D, scl, ramp)
        kw = {} if c["explicit_scale"] is None else {"scaling": c["explicit_scale"]}
        q, k8, v8, sc = _dev(c)
        a = ops.decode_attention_rows_i8kv(q, k8, v8, sc, k8.shape[2], kv_len=_len(s.keys), **kw).cpu().numpy().astype(np.float64)
        b = ops.prefill_attention_i8kv(q, k8, v8, sc, k8.shape[2], kv_len=_len(s.keys), **kw).cpu().numpy().astype(np.float64)
        ratio = np.abs(a - b) / (2.0 * p8.bound8(c["ref"], c["absmean"]))
        assert not np.isnan(a).any() and not np.isnan(b).any() and (ratio <= 1.0).all(), ratio.max()
        worst = max(worst, float(ratio.max()))
    print("attn-rows-i8kv cross-check %s: max ratio %.4f" % (_id(s, n, D), worst))


def test_argument_checks(ops):
    s, D = SHAPES[5], 128
    c = p8.random_case8(s, D, "default", False)
    q, k8, v8, sc = _dev(c)
    call = ops.decode_attention_rows_i8kv
    good = call(q, k8, v8, sc, s.keys, splits=2)
    with pytest.raises(RuntimeError, match="1 .. 16 query rows"):
        call(q.repeat(1, 2, 1, 1), k8, v8, sc, s.keys)
    with pytest.raises(RuntimeError, match="splits must lie in"):
        call(q, k8, v8, sc, s.keys, splits=0)
    with pytest.raises(RuntimeError, match="splits must lie in"):
        call(q, k8, v8, sc, s.keys, splits=MAX_SPLITS + 1)
    with pytest.raises(RuntimeError, match="workspace must be"):
        call(q, k8, v8, sc, s.keys, splits=2,
             workspace=torch.zeros(rows_t.ws_floats(ops, c["q"], s.keys, s.Hkv, 2) - 1, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="kv_len must be"):
        call(q, k8, v8, sc, s.keys, kv_len=torch.tensor([s.keys], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="kv_len_bias needs kv_len"):
        call(q, k8, v8, sc, s.keys, kv_len_bias=1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        call(q, k8, v8, sc, k8.shape[2] + 1)
    with pytest.raises(RuntimeError, match="unsupported head_dim"):
        call(q[..., :32], k8[..., :32], v8[..., :32], sc, s.keys)
    with pytest.raises(RuntimeError, match="int8"):
        call(q, k8.to(torch.float16), v8.to(torch.float16), sc, s.keys)
    with pytest.raises(RuntimeError, match="8 bytes"):           # a cache whose rows are D + 4 bytes apart: the library refuses
        odd = torch.zeros(k8.shape[:3] + (D + 4,), dtype=torch.int8, device=DEV)[..., :D]
        call(q, odd, v8, sc, s.keys)
    torch.cuda.synchronize()
    assert _same_bits(call(q, k8, v8, sc, s.keys, splits=2), good)
