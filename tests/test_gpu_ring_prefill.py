"""The prompt kernel and the prompt's cache write on a ring cache (``ops.prefill_attention`` and
``ops.rotary_embedding_neox_kvcache_prefill`` with ``ring=True``), exact.

A piece of T rows is appended behind ``koff`` logical rows.  The twin is a static cache that holds logical rows 0 .. koff + T - 1 and
goes through the existing ``window=W`` entry; the ring of R = ring_rows(W, T) rows holds logical row r at physical row ``r mod R``
(older rows overwritten by younger ones, never-written rows zero).  The write operator must put the twin's rows koff + t at
``(koff + t) mod R`` and touch nothing else; the attention must return the twin's bits, for the same ``splits``.

koff is chosen so that (a) the piece's own rows cross the ring's end, (b) the piece starts just behind the ring's end, so its lowest
key block lies on the far side of the wrap, (c) the piece lies two turns in at a row that is no multiple of 64.  T in {5, 64, 65, 130}
(one ragged query block, a full half block, one row more, two query blocks), W in {1, 7, 64, 100}, splits in {None -> 1, 2, 3}.
Every case is run a second time with all ring rows the launch does not attend -- never written or stale -- set to a large finite
value: the bits must not move."""
import numpy as np
import pytest
import torch

import attn_cases as ac
from eetq_amd.utils.kv_cache import ring_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, HKV = 2, 4, 2
PIECES = (5, 64, 65, 130)
WINDOWS = (1, 7, 64, 100)
CASES = [(D, T, W) for D in (64, 128) for T in PIECES for W in WINDOWS]
BIG = 60000.0


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.prefill_attention is None:
        pytest.skip("prefill_attention lives in the compiled module")
    return o


def _bits(t):
    return t.contiguous().view(torch.int16)


def _i64(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


_shared = {}


def _data(D):
    """the logical cache rows, the pieces' tokens and the rotary table of a head size (computed once, never changed)"""
    if D not in _shared:
        rng = np.random.default_rng(500 + D)
        t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
        _shared[D] = dict(rows_k=t(ac.normal_f16(rng, (B, HKV, 1024, D))), rows_v=t(ac.nonzero_normal_f16(rng, (B, HKV, 1024, D))),
                          q=t(ac.normal_f16(rng, (B, 130, H, D))), k=t(ac.normal_f16(rng, (B, 130, HKV, D))),
                          v=t(ac.nonzero_normal_f16(rng, (B, 130, HKV, D))), table=t(ac.rope_table(D, 1024)), scale=D ** -0.5)
    return _shared[D]


def koffs(R, T):
    return (R - (T + 1) // 2, R + 3, 2 * R + 61)


def _ring_of(static, koff, R):
    """the ring that holds logical rows 0 .. koff - 1 of `static`: younger rows over older ones, the rest zero"""
    ring = torch.zeros(B, HKV, R, static.shape[3], dtype=torch.float16, device=DEV)
    lo = max(0, koff - R)
    idx = torch.arange(lo, koff, device=DEV)
    ring[:, :, idx % R] = static[:, :, lo:koff]
    return ring


def _setup(ops, D, T, W, koff, R, host_row):
    """write the piece into the twin and into the ring -> (q, twin k, v, ring k, v); checks the write operator on the way"""
    x = _data(D)
    L = koff + T
    tk, tv = x["rows_k"][:, :, :L].clone(), x["rows_v"][:, :, :L].clone()
    tk[:, :, koff:], tv[:, :, koff:] = 0, 0
    rk, rv = _ring_of(tk, koff, R), _ring_of(tv, koff, R)
    before_k, before_v = rk.clone(), rv.clone()
    pos = (koff + torch.arange(T, device=DEV))[None, :].repeat(B, 1).contiguous()
    where = {"first_row": koff} if host_row else {"first_row_dev": _i64([koff])}
    qs = []
    for kc, vc, kw in ((tk, tv, {}), (rk, rv, {"ring": True})):
        q = x["q"][:, :T].clone()
        ops.rotary_embedding_neox_kvcache_prefill(pos, q, x["k"][:, :T].clone(), x["v"][:, :T].clone(), D, x["table"], kc, vc, **where, **kw)
        qs.append(q)
    assert torch.equal(_bits(qs[0]), _bits(qs[1])), "the rotated query"
    new = (koff + torch.arange(T, device=DEV)) % R
    old = torch.ones(R, dtype=torch.bool, device=DEV)
    old[new] = False
    for ring, twin, before in ((rk, tk, before_k), (rv, tv, before_v)):
        assert torch.equal(_bits(ring[:, :, new]), _bits(twin[:, :, koff:L])), "logical row r at physical row r mod R"
        assert torch.equal(_bits(ring[:, :, old]), _bits(before[:, :, old])), "no other physical row changes"
    return qs[0], tk, tv, rk, rv


def _poisoned(ring, koff, T, W, R):
    """the ring with every physical row no query of the launch attends set to BIG"""
    lo = max(0, koff - W + 1)
    keep = torch.zeros(R, dtype=torch.bool, device=DEV)
    keep[torch.arange(lo, koff + T, device=DEV) % R] = True
    out = ring.clone()
    out[:, :, ~keep] = BIG
    return out, int((~keep).sum())


@pytest.mark.parametrize("D", (64, 128))
def test_ring_piece_has_the_bits_of_the_windowed_entry_on_a_static_twin(ops, D):
    """every (T, W) of a head size in one test (the suite counts test items: the cases are a loop, each named in its failure)"""
    for _, T, W in (c for c in CASES if c[0] == D):
        _piece(ops, D, T, W)


def _piece(ops, D, T, W):
    x = _data(D)
    R = ring_rows(W, T)
    assert R % 64 == 0 and W + T + 62 <= R < W + T + 62 + 64
    assert ops.prefill_attention_splits(B, H, T, min(1 << 30, W + min(T, 128))) == 1, "None resolves to one share at these shapes"
    for i, koff in enumerate(koffs(R, T)):
        L = koff + T
        assert koff >= W and L <= 1024
        q, tk, tv, rk, rv = _setup(ops, D, T, W, koff, R, host_row=i == 1)
        pk, n_poisoned = _poisoned(rk, koff, T, W, R)
        pv, _ = _poisoned(rv, koff, T, W, R)
        assert n_poisoned == R - min(R, T + W - 1) > 0
        n = _i64([L])
        for splits in (None, 2, 3):
            where = (D, T, W, koff, splits)
            want = ops.prefill_attention(q, tk, tv, L, scaling=x["scale"], kv_len=n, splits=splits, window=W)
            got = ops.prefill_attention(q, rk, rv, 1 << 30, scaling=x["scale"], kv_len=n, splits=splits, window=W, ring=True)
            assert torch.isfinite(want).all() and torch.equal(_bits(got), _bits(want)), where
            hurt = ops.prefill_attention(q, pk, pv, 1 << 30, scaling=x["scale"], kv_len=n, splits=splits, window=W, ring=True)
            assert torch.equal(_bits(hurt), _bits(want)), (where, "rows outside every window must carry probability 0")
        # the host bound alone (no device length): `keys` is the logical length
        got = ops.prefill_attention(q, rk, rv, L, scaling=x["scale"], splits=2, window=W, ring=True)
        want = ops.prefill_attention(q, tk, tv, L, scaling=x["scale"], splits=2, window=W)
        assert torch.equal(_bits(got), _bits(want)), (D, T, W, koff, "host length")


def test_a_fresh_piece_on_an_empty_ring(ops):
    """koff = 0: rows 0 .. T - 1 of a zeroed ring, the rest never written"""
    D, T, W = 128, 65, 7
    x = _data(D)
    R = ring_rows(W, T)
    q, tk, tv, rk, rv = _setup(ops, D, T, W, 0, R, host_row=True)
    want = ops.prefill_attention(q, tk, tv, T, scaling=x["scale"], window=W)
    got = ops.prefill_attention(q, rk, rv, T, scaling=x["scale"], window=W, ring=True)
    assert torch.equal(_bits(got), _bits(want))


def test_refusals(ops):
    D, T, W = 64, 5, 7
    x = _data(D)
    q = x["q"][:, :T].contiguous()
    ring = lambda rows: torch.zeros(B, HKV, rows, D, dtype=torch.float16, device=DEV)   # noqa: E731
    n = _i64([200])
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.prefill_attention(q, ring(100), ring(100), 1 << 30, kv_len=n, window=W, ring=True)
    with pytest.raises(ValueError, match="too small for window"):
        ops.prefill_attention(q, ring(64), ring(64), 1 << 30, kv_len=n, window=W, ring=True)     # 64 < 7 + 5 + 62
    assert ring_rows(W, T) == 128
    ops.prefill_attention(q, ring(128), ring(128), 1 << 30, kv_len=n, window=W, ring=True)
    with pytest.raises(ValueError, match="ring needs window"):
        ops.prefill_attention(q, ring(128), ring(128), 1 << 30, kv_len=n, ring=True)
    k8 = torch.zeros(B, HKV, 128, D, dtype=torch.int8, device=DEV)
    scales = torch.zeros(B, HKV, 128, 2, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="no ring cache of int8 rows"):
        ops.prefill_attention_i8kv(q, k8, k8.clone(), scales, 128, kv_len=n, ring=True)
    for rows_op in (ops.decode_attention_rows,):
        with pytest.raises(ValueError, match="no ring cache behind the few-row kernel"):
            rows_op(q, ring(128), ring(128), 128, kv_len=n, ring=True)
    with pytest.raises(ValueError, match="no ring cache behind the few-row kernel"):
        ops.decode_attention_rows_i8kv(q, k8, k8.clone(), scales, 128, kv_len=n, ring=True)
    # the write operator: a call's rows must not meet themselves
    pos = torch.arange(T, device=DEV)[None, :].repeat(B, 1).contiguous()
    small = ring(4)
    with pytest.raises(RuntimeError):
        ops.rotary_embedding_neox_kvcache_prefill(pos, q.clone(), x["k"][:, :T].clone(), x["v"][:, :T].clone(), D, x["table"], small,
                                                  small.clone(), ring=True)
    assert not small.any()
