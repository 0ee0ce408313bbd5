"""The decode kernels on a ring cache (``ops.rope_decode_attention`` / ``ops.decode_attention`` /
``ops.rotary_embedding_neox_kvcache`` with ``ring=True``), exact.

A ring of R rows holds logical row r at physical row ``r mod R``.  Its twin is a static cache of L = 3 R + 5 rows driven through the
existing ``window=W`` entries with the same explicit ``splits``.  Both start as zeros and are stepped position by position over the
same random tokens, once through the one-launch form (which writes the new row itself) and once through the unfused pair (the ring
form of the cache-write operator, then the two-launch attention).  At EVERY step: the output bits are the twin's, physical row
``p mod R`` holds the twin's row ``p``, and every other physical row is what it was before the step.  The walk covers n = R - 1, R,
R + 1, 2 R, 3 R and every window that straddles the ring's end.

Shapes: B = 2, 4 / 2 heads, D in {64, 128}; W in {1, 5, 16, 33} with R in {W, 64} and splits in {1, 3}: the twin has at most 197 rows,
below 16 blocks per chunk, so both run the short form.  One LONG case at D = 128: R = 320, W = 300, splits = 1 (20 and 61 blocks in the
one chunk; the rule is restated below and checked, not assumed)."""
import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, HKV = 2, 4, 2
WINDOWS = (1, 5, 16, 33)
SHORT = [(D, W, R, s) for D in (64, 128) for W in WINDOWS for R in sorted({W, 64}) for s in (1, 3)]
LONG = (128, 300, 320, 1)


def long_form(D, rows, splits):
    """attn_decode_shared.hpp, long_chunks: some chunk may own more than kUA + kUB = 16 blocks of 16 (D = 128) or 32 (D = 64) rows"""
    blk = 16 if D == 128 else 32
    return -(-(-(-rows // blk)) // splits) > 16


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


def _bits(t):
    return t.contiguous().view(torch.int16)


def _i64(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


_tokens = {}


def _inputs(D, L):
    """L random tokens of every batch row (shared by the cases of a head size; a prefix is a prefix)"""
    have = _tokens.get(D)
    if have is None or have["L"] < L:
        rng = np.random.default_rng(300 + D)
        t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
        n = max(L, 200)
        have = dict(L=n, q=t(ac.normal_f16(rng, (n, B, H, D))), k=t(ac.normal_f16(rng, (n, B, HKV, D))),
                    v=t(ac.nonzero_normal_f16(rng, (n, B, HKV, D))), table=t(ac.rope_table(D, 1024)),
                    pos=torch.arange(n, dtype=torch.int64, device=DEV)[:, None].repeat(1, B).contiguous(), scale=D ** -0.5)
        _tokens[D] = have
    return have


class _Cache:
    def __init__(self, rows, D):
        self.k = torch.zeros(B, HKV, rows, D, dtype=torch.float16, device=DEV)
        self.v = torch.zeros_like(self.k)
        self.counter = _i64([0])
        self.tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)


def _one_launch(o, x, D, p, c, splits, **kw):
    return o.rope_decode_attention(x["pos"][p], x["q"][p], x["k"][p], x["v"][p], x["table"], c.k, c.v, c.tickets, slots=c.counter,
                                   scaling=x["scale"], splits=splits, kv_len=c.counter, kv_len_bias=1, advance=c.counter, **kw)


def _two_launches(o, x, D, p, c, splits, ring=False, **kw):
    q = x["q"][p].clone()
    rkw = {"ring": True} if ring else {}
    o.rotary_embedding_neox_kvcache(x["pos"][p], q, x["k"][p].clone(), x["v"][p], D, x["table"], c.k, c.v, slots=c.counter, **rkw)
    return o.decode_attention(q, c.k, c.v, scaling=x["scale"], splits=splits, kv_len=c.counter, kv_len_bias=1, advance=c.counter,
                              **rkw, **kw)


def _walk(o, form, D, W, R, splits, steps=None):
    """-> per step [out equal, row written equal (k, v), no other row changed (k, v)] as a bool array [steps, 5].  The walk only
    launches and copies the ring after every step; the comparisons run once, over all steps, when it is over."""
    L = 3 * R + 5
    n = L if steps is None else steps
    x = _inputs(D, L)
    ring, twin = _Cache(R, D), _Cache(L, D)
    snap = {"k": torch.empty((n,) + ring.k.shape, dtype=torch.float16, device=DEV), "v": None}
    snap["v"] = torch.empty_like(snap["k"])
    want, got = [], []
    for p in range(n):
        want.append(form(o, x, D, p, twin, splits, window=W))
        got.append(form(o, x, D, p, ring, splits, window=W, ring=True))
        snap["k"][p].copy_(ring.k)
        snap["v"][p].copy_(ring.v)
    want, got = torch.stack(want), torch.stack(got)
    steps_i = torch.arange(n, device=DEV)
    phys = steps_i % R
    other = torch.arange(R, device=DEV)[None, :] != phys[:, None]                       # [n, R]
    flags = [(_bits(got) == _bits(want)).flatten(1).all(dim=1)]
    for name, cache, static in (("k", ring.k, twin.k), ("v", ring.v, twin.v)):
        after = _bits(snap[name])                                                         # [n, B, Hkv, R, D]: the ring after step p
        before = torch.cat([torch.zeros_like(after[:1]), after[:-1]])                     # ... and before it (zeros at first)
        written = after[steps_i, :, :, phys]                                              # [n, B, Hkv, D]: physical row p mod R
        flags.append((written == _bits(static[:, :, :n]).permute(2, 0, 1, 3)).flatten(1).all(dim=1))
        changed = (after != before).any(dim=4).any(dim=2).any(dim=1)                      # [n, R]
        flags.append(~(changed & other).any(dim=1))
        assert torch.equal(after[-1], _bits(cache))
    flags = torch.stack(flags, dim=1).cpu().numpy()
    assert int(ring.counter.item()) == n == int(twin.counter.item()), "the counters count logical rows"
    assert torch.count_nonzero(ring.tickets) == 0 and torch.isfinite(got).all()
    return flags


def _check(flags, where):
    names = ("output bits", "k row written", "other k rows untouched", "v row written", "other v rows untouched")
    bad = np.argwhere(~flags)
    assert bad.size == 0, (where, "first failure at step %d: %s" % (bad[0][0], names[bad[0][1]]), len(bad))


FORMS = pytest.mark.parametrize("form", (_one_launch, _two_launches), ids=("one", "two"))


@FORMS
def test_ring_has_the_bits_of_the_windowed_entry_on_a_static_twin(ops, form):
    """every (D, W, R, splits) of SHORT in one test of the form (the suite counts test items: the cases are a loop, each named in its
    failure)"""
    for D, W, R, splits in SHORT:
        L = 3 * R + 5
        assert not long_form(D, R, min(splits, R)) and not long_form(D, L, splits), "ring and twin both run the short form"
        if splits > R:   # a one-row ring cannot be cut into three chunks: the entries' own rule (splits <= capacity) refuses it
            c = _Cache(R, D)
            with pytest.raises(RuntimeError, match="invalid attention shape"):
                form(ops, _inputs(D, L), D, 0, c, splits, window=W, ring=True)
            continue
        ops.decode_dropped_steps()
        _check(_walk(ops, form, D, W, R, splits), (form.__name__, D, W, R, splits))
        assert ops.decode_dropped_steps() == 0, "a ring is never full"


@FORMS
def test_ring_long_form(ops, form):
    D, W, R, splits = LONG
    assert long_form(D, R, splits) and long_form(D, 3 * R + 5, splits), "ring and twin both run the LONG form"
    ops.decode_dropped_steps()
    _check(_walk(ops, form, D, W, R, splits), (form.__name__,) + LONG)
    assert ops.decode_dropped_steps() == 0


def test_the_ctypes_binding_walks_the_same_ring(ops):
    import eetq_amd.ops_ctypes as oc
    for form in (_one_launch, _two_launches):
        _check(_walk(oc, form, 64, 5, 64, 3, steps=140), (form.__name__, "ctypes"))


def _attend_only(o, x, D, p, c, splits, **kw):
    return o.decode_attention(x["q"][p], c.k, c.v, scaling=x["scale"], splits=splits, kv_len=c.counter, kv_len_bias=1, advance=c.counter, **kw)


def test_refusals(ops):
    import eetq_amd.ops_ctypes as oc
    D, R = 64, 64
    x = _inputs(D, 8)
    for o in (ops, oc):
        for form in (_one_launch, _attend_only):
            c = _Cache(R, D)
            with pytest.raises(ValueError, match="ring needs window"):
                form(o, x, D, 0, c, 1, ring=True)
            with pytest.raises(ValueError, match="too small for window"):
                form(o, x, D, 0, c, 1, window=R + 1, ring=True)
            with pytest.raises(ValueError, match="kv_start"):
                form(o, x, D, 0, c, 1, window=5, ring=True, kv_start=_i64([0] * B))
            with pytest.raises(ValueError, match="mask"):
                form(o, x, D, 0, c, 1, window=5, ring=True, mask=torch.zeros(B, R, dtype=torch.float16, device=DEV))
            assert int(c.counter.item()) == 0 and not c.k.any() and not c.v.any(), "a refusal writes nothing"
        c = _Cache(R, D)
        with pytest.raises(ValueError, match="ring needs kv_len"):
            o.decode_attention(x["q"][0], c.k, c.v, window=5, ring=True)
