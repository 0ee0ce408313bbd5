"""Prompt attention behind cached rows (eetq_amd/csrc/attn_prefill.hip): the device-length form (the number of keys read from a
device counter, `kv_len` / `kv_len_bias`) and the split-KV form (`splits` workgroups share a workgroup's key blocks, a second
launch merges their records), at D = 128 and D = 64.  Caches are PREFILL_PAD rows longer than `keys` and NaN there; no output
may be NaN.

  device length   bit for bit the host-length call with the same effective keys / causal offset (exact, clamped, biased,
                  Tk < Tq, Tk = 0), in the bshd and fusedq layouts; three chunks of a 320-token prompt reproduce the one call
  split form      the four families of tests/attn_cases.py through the drivers of tests/test_gpu_attn_prefill_edges.py with
                  forced `splits`, against the float64 reference, under the families' own criteria (bit-for-bit V[row] on
                  staircase and pairing, 1 fp16 ulp on the census, attn_cases.random_bound on random data); every call runs
                  once on a NaN-filled and once on a zero-filled workspace and must return the same bits
  together        a split call with the length on the device equals the same split with the host length; splits=None equals
                  the forced call at ops.prefill_attention_splits(...)

Split shapes (SPLIT): the smallest at which the share arithmetic can go wrong; check_split_coverage() restates it (guard only).
The staircase's hot rows straddle every 32- and 64-key edge (edges.edge_rows), so the last row of a share, the first row of the
next and the 63 / 64 / 65 steps are all visited.  T = 129 behind 200 rows (keys 329) is kept as it was asked for although both
of its query blocks have six key blocks; T = 129 behind 192 rows (keys 321) is the shape with five and six.

Largest figures per split case on an MI355X, D = 128 / D = 64 (random: |out - ref| / bound over the four kinds; census: fp16 ulp;
bait: staircase rows before the hot key, |out - ref| / bound):

  case                          random          census            bait
  T40-keys340 splits 2          0.412 / 0.371   0.4985 / 0.4985   0.107 / 0.126
  T40-keys340 splits 3          0.412 / 0.371   0.4985 / 0.4985   0.113 / 0.120
  T40-keys340 splits 4          0.412 / 0.371   0.4985 / 0.4985   0.107 / 0.120
  T40-keys130 splits 8          0.355 / 0.377   0.4961 / 0.4960   0.170 / 0.145
  T1-keys70 splits 2            0.222 / 0.263   0.4857 / 0.4857   (no bait rows)
  T129-keys329 splits 2         0.429 / 0.391   0.4985 / 0.4985   0.129 / 0.143
  T129-keys321 splits 2         0.454 / 0.351   0.4984 / 0.4984   0.130 / 0.138
  T140-keys140-koff-5 splits 2  0.447 / 0.369   0.4963 / 0.4962   0.279 / 0.375

102 cases (the guard among them), 3.8 s wall for the file on an MI355X.
"""
import numpy as np
import pytest
import torch

import attn_cases as ac
import test_gpu_attn_prefill_edges as edges
from test_gpu_attn_prefill_edges import Shape, koff_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = edges.DIMS
BM, BN = edges.BM, edges.BN

ROW2 = edges.ROWS[2][0]          # Shape(2, 200, 8, 4, 237): append behind 37 rows
ROW1 = edges.ROWS[1][0]          # Shape(2, 320, 8, 8, 320)
assert ROW2 == Shape(2, 200, 8, 4, 237, None) and ROW1 == Shape(2, 320, 8, 8, 320, None)

SPLIT = [                                            # (shape, splits)
    (Shape(1, 40, 4, 2, 340, None), 2),              # behind 300 rows, 6 key blocks
    (Shape(1, 40, 4, 2, 340, None), 3),              # ... even shares
    (Shape(1, 40, 4, 2, 340, None), 4),              # ... ragged shares 1, 2, 1, 2
    (Shape(1, 40, 4, 2, 130, None), 8),              # behind 90 rows, 3 key blocks: five shares are empty
    (Shape(1, 1, 2, 2, 70, None), 2),                # one query row behind 69
    (Shape(1, 129, 2, 1, 329, None), 2),             # two query blocks (both with 6 key blocks)
    (Shape(1, 129, 2, 1, 321, None), 2),             # two query blocks with 5 and 6 key blocks
    (Shape(1, 140, 2, 2, 140, -5), 2),               # through kv_len = 135: early rows attend nothing, in any share
]
SPLIT_IDS = ["T%d-keys%d-koff%s-s%d" % (s.T, s.keys, "dflt" if s.koff is None else s.koff, n) for s, n in SPLIT]


# ---- the share arithmetic, restated (guard only) ---------------------------------------------------------------------------

def shares(s, ns):
    """[(query block, nblk, [(j0, j1) of every share])]"""
    out = []
    for qb, nblk, _ in edges.geometry(s):
        out.append((qb, nblk, [(i * nblk // ns, (i + 1) * nblk // ns) for i in range(ns)]))
    return out


def check_split_coverage():
    def sizes(s, ns):
        return [[b - a for a, b in sh] for _, _, sh in shares(s, ns)]
    (a2, _), (a3, _), (a4, _), (b8, _), (c2, _), (d2, _), (e2, _), (f2, _) = SPLIT
    assert a2 == a3 == a4 and koff_of(a2) == 300 and sizes(a2, 2) == [[3, 3]] and sizes(a3, 3) == [[2, 2, 2]]
    assert sizes(a4, 4) == [[1, 2, 1, 2]], "ragged"
    assert koff_of(b8) == 90 and sizes(b8, 8) == [[0, 0, 1, 0, 0, 1, 0, 1]], "five empty shares"
    assert c2.T == 1 and koff_of(c2) == 69 and sizes(c2, 2) == [[1, 1]]
    assert koff_of(d2) == 200 and sizes(d2, 2) == [[3, 3], [3, 3]]
    assert koff_of(e2) == 192 and sizes(e2, 2) == [[2, 3], [3, 3]], "two query blocks with different nblk"
    assert sizes(f2, 2) == [[1, 1], [1, 2]] and (ac.prefill_counts(f2.T, f2.keys, f2.koff) == 0).sum() == 5
    # rows 5 .. 63 of the koff = -5 shape attend keys of the first block only: nothing in the second share
    assert ac.prefill_counts(f2.T, f2.keys, f2.koff)[63] == 59 <= BN
    for s, ns in SPLIT:     # every share boundary is a 64-key edge the staircase straddles
        rows = set(edges.edge_rows(s.keys))
        for _, _, sh in shares(s, ns):
            for a, b in sh:
                for r in (a * BN - 1, a * BN, a * BN + 1) if a > 0 else ():
                    assert r in rows or not 0 <= r < s.keys
    assert all(s.keys <= 340 and s.T <= 140 for s, _ in SPLIT)


def test_split_coverage_guard():
    check_split_coverage()


# ---- the GPU side ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.prefill_attention is None:
        pytest.skip("prefill_attention lives in the compiled module")
    return o


def _len(n):
    return torch.tensor([n], dtype=torch.int64, device=DEV)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def ws_floats(q, splits):
    B, T, H, D = q.shape
    return B * H * T * splits * (D + 2)


def split_attend(ops, splits, device_length=False, layout="plain"):
    """attend(q, k, v, keys, koff, scale) of the family drivers through the split form with `splits` forced; a causal offset
    other than keys - T goes through kv_len = T + koff.  Runs on a NaN-filled and on a zero-filled workspace."""
    def attend(q, k, v, keys, koff, scale):
        T = q.shape[1]
        kw = {} if scale is None else {"scaling": scale}
        if device_length or (koff is not None and koff != keys - T):
            n = keys if koff is None else T + koff
            assert 0 <= n <= keys
            kw["kv_len"] = _len(n)
        qd, kd, vd = edges._lay_q(q, layout), edges._lay_kv(k, layout), edges._lay_kv(v, layout)
        outs = []
        for fill in (float("nan"), 0.0):
            ws = torch.full((ws_floats(q, splits),), fill, dtype=torch.float32, device=DEV)
            outs.append(ops.prefill_attention(qd, kd, vd, keys, splits=splits, workspace=ws, **kw))
        assert _same_bits(outs[0], outs[1]), "the result depends on what the workspace held"
        assert outs[0].shape == q.shape and outs[0].is_contiguous()
        return outs[0].cpu().numpy()
    return attend


CASES = [(i, D) for i in range(len(SPLIT)) for D in DIMS]
CASE_IDS = ["%s-D%d" % (SPLIT_IDS[i], D) for i, D in CASES]
PAIRED = [(i, D) for i, D in CASES if SPLIT[i][0].koff is None]       # pairing needs t + koff >= 0 for every t
PAIRED_IDS = ["%s-D%d" % (SPLIT_IDS[i], D) for i, D in PAIRED]


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_split_staircase_across_share_boundaries(ops, i, D):
    s, ns = SPLIT[i]
    worst = edges.drive_staircase_edges(split_attend(ops, ns), s, D)
    print("prefill-append staircase-bait %s D=%d: max ratio %.3f" % (SPLIT_IDS[i], D, worst))


@pytest.mark.parametrize("kind", ("diagonal", "permutation"))
@pytest.mark.parametrize("i,D", PAIRED, ids=PAIRED_IDS)
def test_split_pairing(ops, i, D, kind):
    s, ns = SPLIT[i]
    edges.drive_pairing(split_attend(ops, ns), s, D, kind)


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_split_prefix_census(ops, i, D):
    s, ns = SPLIT[i]
    worst = edges.drive_census(split_attend(ops, ns), s, D)
    print("prefill-append census %s D=%d: max error %.4f ulp" % (SPLIT_IDS[i], D, worst))


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_split_random(ops, i, D):
    s, ns = SPLIT[i]
    worst = max(edges.drive_random(split_attend(ops, ns), s, D, scaling, ramp) for scaling, ramp in edges.RANDOM_KINDS)
    print("prefill-append random %s D=%d: max ratio %.4f" % (SPLIT_IDS[i], D, worst))


@pytest.mark.parametrize("D", DIMS)
def test_split_with_device_length_equals_split_with_host_length(ops, D):
    s, ns = SPLIT[1]
    assert (s.keys, ns) == (340, 3)
    c = edges.random_case(s, D, "default", True)
    host = split_attend(ops, ns)(c["q"], c["k"], c["v"], s.keys, None, None)
    dev = split_attend(ops, ns, device_length=True)(c["q"], c["k"], c["v"], s.keys, None, None)
    assert not np.isnan(host).any() and np.array_equal(host.view(np.int16), dev.view(np.int16))


@pytest.mark.parametrize("i,D", CASES, ids=CASE_IDS)
def test_default_rule_equals_the_forced_call(ops, i, D):
    """splits=None (with the length on the device, which is what selects the new entry point) takes
    ops.prefill_attention_splits(B, H, T, keys) shares."""
    s, _ = SPLIT[i]
    c = edges.random_case(s, D, "default", False)
    q, k, v = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k", "v"))
    n = s.keys if s.koff is None else s.T + s.koff
    rule = ops.prefill_attention_splits(s.B, s.H, s.T, s.keys)
    assert 1 <= rule <= 16
    a = ops.prefill_attention(q, k, v, s.keys, kv_len=_len(n))
    b = ops.prefill_attention(q, k, v, s.keys, kv_len=_len(n), splits=rule)
    assert not torch.isnan(a).any() and _same_bits(a, b)


# ---- device length ---------------------------------------------------------------------------------------------------------------

LENGTHS = [                      # (name, kv_len, bias, the host call's keys: its causal offset is keys - T)
    ("exact", 237, 0, 237),
    ("biased", 230, 7, 237),
    ("clamped", 10000, 0, 237),
    ("short", 195, 0, 195),      # Tk < Tq: the first five rows have nothing to attend
]


@pytest.mark.parametrize("layout", ("bshd", "fusedq"))
@pytest.mark.parametrize("D", DIMS)
def test_device_length_equals_host_length_bit_for_bit(ops, D, layout):
    s = ROW2
    c = edges.random_case(s, D, "default", True)
    q, k, v = edges._lay_q(c["q"], layout), edges._lay_kv(c["k"], layout), edges._lay_kv(c["v"], layout)
    for name, n, bias, keys in LENGTHS:
        host = ops.prefill_attention(q, k, v, keys)
        dev = ops.prefill_attention(q, k, v, s.keys, kv_len=_len(n), kv_len_bias=bias)
        assert not torch.isnan(dev).any(), name
        assert _same_bits(host, dev), name
        if name == "short":
            assert not dev[:, :5].any() and dev[:, 5].any()
    zero = ops.prefill_attention(q, k, v, s.keys, kv_len=_len(9), kv_len_bias=-9)
    assert zero.shape == c["q"].shape and not zero.any() and not torch.isnan(zero).any()
    below = ops.prefill_attention(q, k, v, s.keys, kv_len=_len(-3))
    assert not below.any()


@pytest.mark.parametrize("D", DIMS)
def test_chunks_equal_the_whole_bit_for_bit(ops, D):
    """A 320-token prompt in one fresh call, and as query rows [0, 77), [77, 205), [205, 320) with the device length at 77, 205 and
    320 on the same cache."""
    s = ROW1
    c = edges.random_case(s, D, "default", True)
    q, k, v = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k", "v"))
    whole = ops.prefill_attention(q, k, v, s.keys)
    assert not torch.isnan(whole).any()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    for c0, c1 in ((0, 77), (77, 205), (205, 320)):
        counter.fill_(c1)
        part = ops.prefill_attention(q[:, c0:c1], k, v, s.keys, kv_len=counter)
        assert _same_bits(part, whole[:, c0:c1]), (c0, c1)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(ops):
    s, D = SPLIT[0][0], 64
    c = edges.random_case(s, D, "default", False)
    q, k, v = (torch.from_numpy(c[x]).to(DEV) for x in ("q", "k", "v"))
    good = ops.prefill_attention(q, k, v, s.keys, kv_len=_len(s.keys), splits=2)
    with pytest.raises(RuntimeError, match="causal_offset"):
        ops.prefill_attention(q, k, v, s.keys, causal_offset=300, kv_len=_len(s.keys))
    with pytest.raises(RuntimeError, match="kv_len"):
        ops.prefill_attention(q, k, v, s.keys, kv_len=torch.tensor([s.keys], dtype=torch.int64))             # on the host
    with pytest.raises(RuntimeError, match="kv_len"):
        ops.prefill_attention(q, k, v, s.keys, kv_len=torch.tensor([s.keys], dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="workspace"):
        ops.prefill_attention(q, k, v, s.keys, splits=2, workspace=torch.zeros(ws_floats(c["q"], 2) - 1, dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match="workspace"):
        ops.prefill_attention(q, k, v, s.keys, splits=2, workspace=torch.zeros(ws_floats(c["q"], 2), dtype=torch.float16, device=DEV))
    with pytest.raises(RuntimeError, match="splits"):
        ops.prefill_attention(q, k, v, s.keys, splits=0)
    with pytest.raises(RuntimeError, match="splits"):
        ops.prefill_attention(q, k, v, s.keys, splits=17)
    torch.cuda.synchronize()
    again = ops.prefill_attention(q, k, v, s.keys, kv_len=_len(s.keys), splits=2)
    assert _same_bits(good, again)
