"""Few-row attention behind a long cache (``ops.decode_attention_rows``, eetq_amd/csrc/attn_decode_rows.hip): the four prompt
families of tests/attn_cases.py through the drivers of tests/test_gpu_attn_prefill_edges.py, with ``kv_len`` on the device, at the
smallest shapes at which this kernel can go wrong, D = 128 and D = 64.

  staircase, pairing   out[t] == V[row] BIT FOR BIT
  census               within 1 fp16 ulp of the float64 mean
  random               |out - ref| <= attn_cases.random_bound against the float64 prefill_reference

Every cache carries PREFILL_PAD NaN rows behind ``keys``; no output may be NaN.  Every call runs on a NaN-filled and on a zero-filled
workspace and must give the same bits.  The chunk rule of include/eetq_amd.h is restated here (``chunks``; guard only, never a
source of expected values): chunk i of `splits` owns the 32-row blocks [i n / splits, (i + 1) n / splits) of n = ceil(keys / 32).

Shapes (B, R, H, Hkv, keys) and what each reaches: see SHAPES.  The 1101-key row needs no more keys for this geometry: at its default
8 chunks a chunk holds 4 - 5 blocks, so a workgroup's first wave takes a second trip -- the prefetched prologue and the steady loop
(check_chunk_coverage asserts it).

262 cases (the guard among them), 5.2 s wall for the file on an MI355X.  Largest figures over all shapes and chunk counts,
D = 128 / D = 64:

  random: |out - ref| / bound                                       0.387 / 0.415
  census: error in fp16 ulp                                         0.4985 / 0.4985
  staircase bait rows: |out - ref| / bound                          0.345 / 0.382
  cross-check: |rows - prompt| / (the sum of the two bounds)        0.324 / 0.247
"""
import numpy as np
import pytest
import torch

import attn_cases as ac
import test_gpu_attn_prefill_edges as edges
from test_gpu_attn_prefill_edges import Shape

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = edges.DIMS
BLK = 32            # the kernel's key block
MAX_SPLITS = 64

# Shape(B, T = R, H, Hkv, keys, koff = None: keys - R)
SHAPES = [
    Shape(2, 2, 4, 2, 2, None),        # empty cache, two rows
    Shape(1, 16, 4, 4, 16, None),      # empty cache, a full 16-row tile, MHA
    Shape(2, 5, 8, 2, 69, None),       # behind 64 rows; 4 heads per kv head x 5 rows = 20 tile rows: a second, partly filled sub-tile
    Shape(1, 16, 4, 1, 80, None),      # 64 tile rows: the widest tile
    Shape(2, 3, 2, 2, 130, None),      # keys % 64 = 2: the descriptor-range case of ADVICE.md
    Shape(1, 9, 4, 2, 340, None),      # behind 331 rows, several chunks
    Shape(1, 16, 2, 1, 528, None),     # behind 512 rows
    Shape(1, 2, 2, 2, 1101, None),     # a chunk long enough for the steady loop
    Shape(1, 1, 2, 2, 70, None),       # one row
    Shape(1, 5, 2, 2, 3, None),        # keys < R: queries 0 and 1 attend nothing; census and random only
]
SHORT = Shape(1, 5, 2, 2, 3, None)
NO_RAMP = Shape(2, 5, 8, 2, 69, None)  # the ramp generator finds no rising draw here
FORCED = {130: (1, 2, 3, MAX_SPLITS), 340: (1, 2, 3, MAX_SPLITS), 528: (1, 2, 3, MAX_SPLITS)}


def splits_of(s):
    """the split counts a shape runs at: None (the library's rule) everywhere, forced ones on three shapes"""
    return (None,) + FORCED.get(s.keys, ())


PAIRS = [(s, n) for s in SHAPES for n in splits_of(s)]


def _id(s, n=None, D=None):
    return "B%d-R%d-H%d-%d-keys%d%s%s" % (s.B, s.T, s.H, s.Hkv, s.keys, "" if n is None else "-s%d" % n, "" if D is None else "-D%d" % D)


# ---- the chunk rule, restated (guard only) -----------------------------------------------------------------------------------

def chunks(keys, splits):
    """[(first key row, end key row) of every chunk]"""
    n = -(-keys // BLK)
    return [(BLK * (i * n // splits), min(keys, BLK * ((i + 1) * n // splits))) for i in range(splits)]


def default_splits(s):
    """the library's rule (a pure host function) for the calls below, whose max_keys is the whole cache, NaN rows included;
    through ctypes so that tests/test_attn_rows_cpu.py can ask too"""
    from eetq_amd import _lib
    return _lib.lib().eetq_decode_attention_rows_splits(s.B, s.H, s.Hkv, s.T, s.keys + ac.PREFILL_PAD)


def check_chunk_coverage():
    for s, n in PAIRS:
        ns = default_splits(s) if n is None else n
        assert 1 <= ns <= MAX_SPLITS
        ch = chunks(s.keys, ns)
        owner = np.zeros(s.keys, dtype=np.int64)
        for a, b in ch:
            owner[a:b] += 1
        assert (owner == 1).all(), "every key row belongs to exactly one chunk"
    sizes = lambda keys, ns: [max(0, b - a) for a, b in chunks(keys, ns)]
    assert sizes(130, MAX_SPLITS).count(0) == MAX_SPLITS - 5 and sorted(x for x in sizes(130, MAX_SPLITS) if x) == [2, 32, 32, 32, 32]
    assert sizes(340, 3) == [96, 128, 116] and sizes(340, 2) == [160, 180], "ragged chunks"
    assert sizes(528, 3) == [160, 192, 176] and 32 in sizes(528, MAX_SPLITS), "a one-block chunk"
    assert 0 in sizes(340, MAX_SPLITS) and 32 in sizes(340, MAX_SPLITS) and 20 in sizes(340, MAX_SPLITS)
    long = Shape(1, 2, 2, 2, 1101, None)
    assert max(sizes(1101, default_splits(long))) > 4 * BLK, "some wave of a chunk takes a second trip"


def test_chunk_coverage_guard():
    check_chunk_coverage()


# ---- this file's hot rows ----------------------------------------------------------------------------------------------------

def hot_rows(s, ns):
    """row 0 and the last row, the rows around every multiple of the key block and around every chunk boundary, the whole
    causal tail koff - 1 .. keys - 1"""
    koff = s.keys - s.T
    rows = [0, s.keys - 1] + list(range(koff - 1, s.keys))
    for e in list(range(BLK, s.keys + 1, BLK)) + [a for a, _ in chunks(s.keys, ns)]:
        rows += [e - 1, e, e + 1]
    return sorted(set(r for r in rows if 0 <= r < s.keys))


def two_step_pairs(s, ns):
    """(r1 < r2): across a block edge, across a chunk boundary, inside the causal tail, the two ends"""
    koff = s.keys - s.T
    pairs = [(BLK - 1, BLK), (2 * BLK - 2, 2 * BLK + 1), (0, s.keys - 1), (koff, koff + 1), (koff - 1, s.keys - 1), (s.keys - 2, s.keys - 1)]
    for a, _ in chunks(s.keys, ns):
        pairs += [(a - 1, a), (a - 2, a + 1)]
    return sorted(set((a, b) for a, b in pairs if 0 <= a < b < s.keys))


def drive_edge_rows(attend, s, D, ns):
    c = edges.staircase_case(s, D)
    heads, worst = s.B * s.Hkv, 0.0
    rows = hot_rows(s, ns)
    for i in range(0, len(rows), heads):
        r = np.resize(np.array(rows[i: i + heads]), heads).reshape(s.B, s.Hkv)
        bad, ratio = edges._steps_launch(attend, s, c, [(r, c["hot"], 1)])
        worst = max(worst, ratio)
        assert not bad.any(), "hot rows %s: %s" % (r.reshape(-1).tolist(), edges._first(bad, "query rows"))
    pairs = two_step_pairs(s, ns)
    for i in range(0, len(pairs), heads):
        pr = np.resize(np.array(pairs[i: i + heads]), (heads, 2))
        r1, r2 = pr[:, 0].reshape(s.B, s.Hkv), pr[:, 1].reshape(s.B, s.Hkv)
        for first, second, name in ((("hot", 1), ("hotter", 2), "hot then hotter"), (("hotter", 2), ("hot", 1), "hotter then hot")):
            bad, ratio = edges._steps_launch(attend, s, c, [(r1, c[first[0]], first[1]), (r2, c[second[0]], second[1])])
            worst = max(worst, ratio)
            assert not bad.any(), "%s at %s: %s" % (name, pr.tolist(), edges._first(bad, "query rows"))
    return worst


# ---- the GPU side ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.BOUNDARY != "ext":
        pytest.skip("decode_attention_rows lives in the compiled module")
    assert o.decode_attention_rows is not None and o.decode_attention_rows_splits is not None
    return o


def _len(n):
    return torch.tensor([n], dtype=torch.int64, device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def ws_floats(ops, q, keys, Hkv, splits):
    B, R, H, D = q.shape
    ns = ops.decode_attention_rows_splits(B, H, Hkv, R, keys) if splits is None else splits
    return B * H * R * ns * (D + 4)


def rows_attend(ops, splits=None, layout="plain"):
    """attend(q, k, v, keys, koff, scale) of the family drivers: kv_len on the device, koff = None.  Twice, on a NaN-filled and on a
    zero-filled workspace, then once more on the first: equal bits."""
    def attend(q, k, v, keys, koff, scale):
        assert koff is None
        kw = {} if scale is None else {"scaling": scale}
        qd, kd, vd = edges._lay_q(q, layout), edges._lay_kv(k, layout), edges._lay_kv(v, layout)
        n = ws_floats(ops, q, kd.shape[2], k.shape[1], splits)
        outs = []
        for fill in (float("nan"), 0.0, float("nan")):
            ws = torch.full((n,), fill, dtype=torch.float32, device=DEV)
            outs.append(ops.decode_attention_rows(qd, kd, vd, kd.shape[2], kv_len=_len(keys), splits=splits, workspace=ws, **kw))
        assert _same_bits(outs[0], outs[1]), "the result depends on what the workspace held"
        assert _same_bits(outs[0], outs[2]), "a repeated call gives other bits"
        assert outs[0].shape == q.shape and outs[0].is_contiguous()
        return outs[0].cpu().numpy()
    return attend


def _params(pairs):
    return [(s, n, D) for s, n in pairs for D in DIMS]


def _ids(params):
    return [_id(s, n, D) for s, n, D in params]


SWEEP = _params([(s, None) for s in SHAPES if s.keys <= 80 and s != SHORT])
HOT = _params([(s, n) for s, n in PAIRS if s != SHORT])
ALL = _params(PAIRS)


@pytest.mark.parametrize("s,n,D", SWEEP, ids=_ids(SWEEP))
def test_staircase_every_row(ops, s, n, D):
    worst = edges.drive_staircase_sweep(rows_attend(ops, n), s, D)
    print("attn-rows staircase-bait sweep %s: max ratio %.3f" % (_id(s, n, D), worst))


@pytest.mark.parametrize("s,n,D", HOT, ids=_ids(HOT))
def test_staircase_edge_rows_and_two_steps(ops, s, n, D):
    ns = default_splits(s) if n is None else n
    worst = drive_edge_rows(rows_attend(ops, n), s, D, ns)
    print("attn-rows staircase-bait edges %s: max ratio %.3f" % (_id(s, n, D), worst))


@pytest.mark.parametrize("kind", ("diagonal", "permutation"))
@pytest.mark.parametrize("s,n,D", HOT, ids=_ids(HOT))
def test_pairing(ops, s, n, D, kind):
    edges.drive_pairing(rows_attend(ops, n), s, D, kind)


@pytest.mark.parametrize("s,n,D", ALL, ids=_ids(ALL))
def test_prefix_census(ops, s, n, D):
    worst = edges.drive_census(rows_attend(ops, n), s, D)
    print("attn-rows census %s: max error %.4f ulp" % (_id(s, n, D), worst))


def random_kinds(s):
    return [(sc, ramp) for sc, ramp in edges.RANDOM_KINDS if not (ramp and s == NO_RAMP)]


@pytest.mark.parametrize("s,n,D", ALL, ids=_ids(ALL))
def test_random(ops, s, n, D):
    worst = max(edges.drive_random(rows_attend(ops, n), s, D, sc, ramp) for sc, ramp in random_kinds(s))
    print("attn-rows random %s: max ratio %.4f" % (_id(s, n, D), worst))


LAYOUT_SHAPES = [Shape(2, 5, 8, 2, 69, None), Shape(2, 3, 2, 2, 130, None)]


@pytest.mark.parametrize("layout", edges.LAYOUTS)
@pytest.mark.parametrize("s", LAYOUT_SHAPES, ids=[_id(s) for s in LAYOUT_SHAPES])
@pytest.mark.parametrize("D", DIMS)
def test_layouts(ops, s, D, layout):
    """the strided query view of a fused QKV row, [B, S, Hkv, D] cache storage, cache rows D + 8 apart"""
    attend = rows_attend(ops, None, layout)
    drive_edge_rows(attend, s, D, default_splits(s))
    edges.drive_pairing(attend, s, D, "diagonal")
    edges.drive_census(attend, s, D)
    edges.drive_random(attend, s, D, "default", False)


DEVLEN = [Shape(1, 9, 4, 2, 340, None), Shape(2, 3, 2, 2, 130, None)]


@pytest.mark.parametrize("s", DEVLEN, ids=[_id(s) for s in DEVLEN])
@pytest.mark.parametrize("D", DIMS)
def test_device_length(ops, s, D):
    """A cache with more rows than *kv_len, kv_len_bias != 0, *kv_len beyond max_keys (clamped), *kv_len = 0 (zeros): each equals the
    call with the effective keys passed as max_keys and kv_len=None, bit for bit (the same chunk count: the chunks follow the keys)."""
    c = edges.random_case(s, D, "default", True)
    q, k, v = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k", "v"))
    rows = k.shape[2]
    assert rows == s.keys + ac.PREFILL_PAD
    for ns in (1, 3):
        for n, bias, mk, eff in ((s.keys, 0, rows, s.keys), (s.keys - 40, 0, rows, s.keys - 40), (s.keys - 7, 5, rows, s.keys - 2),
                                 (s.keys + 3, -20, rows, s.keys - 17), (s.keys + 1000, 0, s.keys, s.keys), (rows, 2, s.keys - 1, s.keys - 1),
                                 (5, 0, rows, 5)):
            host = ops.decode_attention_rows(q, k, v, eff, splits=ns)
            dev = ops.decode_attention_rows(q, k, v, mk, kv_len=_len(n), kv_len_bias=bias, splits=ns)
            assert not torch.isnan(dev).any()
            assert _same_bits(host, dev), (ns, n, bias, mk)
        zero = ops.decode_attention_rows(q, k, v, rows, kv_len=_len(0), splits=ns)
        below = ops.decode_attention_rows(q, k, v, rows, kv_len=_len(9), kv_len_bias=-12, splits=ns)
        assert not zero.any() and not below.any() and not torch.isnan(zero).any()


CROSS = _params([(s, None) for s in SHAPES])


@pytest.mark.parametrize("s,n,D", CROSS, ids=_ids(CROSS))
def test_cross_check_against_the_prompt_kernel(ops, s, n, D):
    """|rows - prompt| <= the sum of the two calls' random bounds (not bit equality: the tiles differ)"""
    worst = 0.0
    for sc, ramp in random_kinds(s):
        c = edges.random_case(s, D, sc, ramp)
        kw = {} if c["explicit_scale"] is None else {"scaling": c["explicit_scale"]}
        q, k, v = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k", "v"))
        a = ops.decode_attention_rows(q, k, v, k.shape[2], kv_len=_len(s.keys), **kw).cpu().numpy().astype(np.float64)
        b = ops.prefill_attention(q, k, v, k.shape[2], kv_len=_len(s.keys), **kw).cpu().numpy().astype(np.float64)
        ratio = np.abs(a - b) / (2.0 * ac.random_bound(c["ref"], c["absmean"]))
        assert not np.isnan(a).any() and (ratio <= 1.0).all(), ratio.max()
        worst = max(worst, float(ratio.max()))
    print("attn-rows cross-check %s: max ratio %.4f" % (_id(s, n, D), worst))


def test_argument_checks(ops):
    s, D = SHAPES[5], 128
    c = edges.random_case(s, D, "default", False)
    q, k, v = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k", "v"))
    good = ops.decode_attention_rows(q, k, v, s.keys, splits=2)
    with pytest.raises(RuntimeError, match="1 .. 16 query rows"):
        ops.decode_attention_rows(q.repeat(1, 2, 1, 1), k, v, s.keys)
    with pytest.raises(RuntimeError, match="splits must lie in"):
        ops.decode_attention_rows(q, k, v, s.keys, splits=0)
    with pytest.raises(RuntimeError, match="splits must lie in"):
        ops.decode_attention_rows(q, k, v, s.keys, splits=MAX_SPLITS + 1)
    with pytest.raises(RuntimeError, match="workspace must be"):
        ops.decode_attention_rows(q, k, v, s.keys, splits=2, workspace=torch.zeros(ws_floats(ops, c["q"], s.keys, s.Hkv, 2) - 1,
                                                                                   dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="kv_len must be"):
        ops.decode_attention_rows(q, k, v, s.keys, kv_len=torch.tensor([s.keys], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="kv_len_bias needs kv_len"):
        ops.decode_attention_rows(q, k, v, s.keys, kv_len_bias=1)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.decode_attention_rows(q, k, v, k.shape[2] + 1)
    with pytest.raises(RuntimeError, match="unsupported head_dim"):
        ops.decode_attention_rows(q[..., :32], k[..., :32], v[..., :32], s.keys)
    assert _same_bits(ops.decode_attention_rows(q, k, v, s.keys, splits=2), good)
