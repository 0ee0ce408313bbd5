"""The attention kernels with a per-row first key (``kv_start``), all exact: a left-padded batch row must come out with the
BITS of the existing entry called on that row alone, moved to its first real token.

Prompt attention (``ops.prefill_attention(..., kv_start=)``, eetq_prefill_attention_padded_f16): row b with p pad queries and its
first real cache row s is compared with ``ops.prefill_attention`` on ``q[b, p:]`` and ``k[b, :, s:]`` -- the same splits, the same
length form -- bit for bit; ``out[b, :p]`` is zeros; the cache rows below s, the rows beyond the keys and the pad QUERY rows are
NaN, so a single read of any of them shows.  Decode attention (``ops.rope_decode_attention`` / ``ops.decode_attention`` with
``kv_start``): row b is compared with the existing entry on a cache of the same capacity whose rows [0, S - s) are this cache's
rows [s, S), with the counter and the mask moved by s; the rows below s and beyond the slot hold a NaN byte pattern that must
neither change nor reach the output.

Shapes are the smallest that reach every path: starts on both sides of the key blocks (64), query blocks (128) and decode blocks
(16 rows at D = 128, 32 at D = 64), more than one block per chunk, the LONG instantiation at both head sizes, forced splits."""
import numpy as np
import pytest
import torch

import attn_cases as ac
import test_gpu_attn_prefill_edges as edges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (128, 64)
B_PF, H, HKV, T = 4, 4, 2, 200
NAN_BITS = 0x7E7E            # an fp16 NaN whose two bytes are equal: the sentinel of rows nobody may touch


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


# ==== prompt attention ==========================================================================================================
# every start of {0, 1, 63, 64, 65, 127, 128, 129, 199}, mixed within a batch, a 0 in every batch
START_BATCHES = ((0, 1, 63, 64), (65, 0, 127, 128), (129, 199, 0, 64))
# (name, keys, length on the device, splits, batches of starts): `keys - T` rows are cached in front of the prompt
PREFILL_CASES = (
    ("fresh", T, False, 1, START_BATCHES),
    ("behind37", T + 37, True, 1, START_BATCHES),
    # behind 300 rows the starts above are all pads in the cached rows alone (p = 0): half of them move into the prompt
    ("behind300_s2", T + 300, True, 2, ((0, 301, 63, 364), (365, 0, 427, 128), (429, 499, 0, 64))),
    ("behind300_s3", T + 300, True, 3, ((0, 301, 63, 364), (365, 0, 427, 128), (429, 499, 0, 64))),
    # a start at or beyond the end of the piece: the whole piece of that row is pads
    ("allpad", T + 37, True, 1, ((0, 237, 250, 100),)),
    ("allpad_s2", T + 37, True, 2, ((0, 237, 250, 100),)),
)


def _prefill_inputs(D, keys, seed):
    rng = np.random.default_rng(seed)
    q = ac.normal_f16(rng, (B_PF, T, H, D))
    k = ac.poison_tail(ac.normal_f16(rng, (B_PF, HKV, keys + ac.PREFILL_PAD, D)), keys)
    v = ac.poison_tail(ac.normal_f16(rng, (B_PF, HKV, keys + ac.PREFILL_PAD, D)), keys)
    return q, k, v


def _prefill_call(ops, q, k, v, keys, on_device, splits, **kw):
    if on_device:
        kw["kv_len"] = _i64(keys)
    if on_device or splits > 1:
        kw["splits"] = splits
    return ops.prefill_attention(q, k, v, keys, **kw)


@pytest.mark.parametrize("layout", ("plain", "fusedq"))
@pytest.mark.parametrize("case", PREFILL_CASES, ids=[c[0] for c in PREFILL_CASES])
@pytest.mark.parametrize("D", DIMS)
def test_prefill_rows_have_the_bits_of_the_shifted_single_row(ops, D, case, layout):
    name, keys, on_device, splits, batches = case
    koff = keys - T
    q_np, k_np, v_np = _prefill_inputs(D, keys, seed=7 * keys + D + splits)
    for starts in batches:
        pads = [min(T, max(0, s - koff)) for s in starts]
        qn, kn, vn = q_np.copy(), k_np.copy(), v_np.copy()
        for b, (s, p) in enumerate(zip(starts, pads)):       # NaN wherever the row's contract says "not read"
            kn[b, :, :min(s, keys)] = np.float16(np.nan)
            vn[b, :, :min(s, keys)] = np.float16(np.nan)
            qn[b, :p] = np.float16(np.nan)
        q = edges._lay_q(qn, layout)
        k, v = torch.from_numpy(kn).to(DEV), torch.from_numpy(vn).to(DEV)
        out = _prefill_call(ops, q, k, v, keys, on_device, splits, kv_start=_i64(starts))
        assert out.shape == (B_PF, T, H, D) and out.is_contiguous()
        assert not torch.isnan(out).any(), (name, starts)
        for b, (s, p) in enumerate(zip(starts, pads)):
            assert torch.count_nonzero(_bits(out[b, :p])) == 0, (name, starts, b, "pad queries must be zeros")
            if p == T:
                continue
            want = _prefill_call(ops, q[b:b + 1, p:], k[b:b + 1, :, s:], v[b:b + 1, :, s:], keys - s, on_device, splits)
            assert torch.equal(_bits(out[b, p:]), _bits(want[0])), (name, starts, b)


@pytest.mark.parametrize("case", PREFILL_CASES[:4], ids=[c[0] for c in PREFILL_CASES[:4]])
@pytest.mark.parametrize("D", DIMS)
def test_prefill_all_starts_zero_is_the_existing_entry(ops, D, case):
    name, keys, on_device, splits, _ = case
    q_np, k_np, v_np = _prefill_inputs(D, keys, seed=3 * keys + D)
    q, k, v = (torch.from_numpy(x).to(DEV) for x in (q_np, k_np, v_np))
    got = _prefill_call(ops, q, k, v, keys, on_device, splits, kv_start=_i64([0] * B_PF))
    want = _prefill_call(ops, q, k, v, keys, on_device, splits)
    assert torch.isfinite(want).all() and torch.equal(_bits(got), _bits(want))


def test_prefill_kv_start_is_checked(ops):
    q_np, k_np, v_np = _prefill_inputs(64, T, seed=1)
    q, k, v = (torch.from_numpy(x).to(DEV) for x in (q_np, k_np, v_np))
    for bad in (torch.zeros(B_PF, dtype=torch.int32, device=DEV), torch.zeros(B_PF + 1, dtype=torch.int64, device=DEV),
                torch.zeros(B_PF, dtype=torch.int64), torch.zeros(2 * B_PF, dtype=torch.int64, device=DEV)[::2]):
        with pytest.raises(RuntimeError, match="kv_start"):
            ops.prefill_attention(q, k, v, T, kv_start=bad)


# ==== decode attention ==========================================================================================================
B_DEC = 3
# (D, S, splits): splits = 1 at S = 320 is the LONG instantiation at D = 128 (20 blocks of 16 > 16), S = 576 at D = 64 (18 blocks of
# 32); the others are not LONG, S = 256 among them
DECODE_CASES = ((128, 320, 1), (128, 320, 3), (128, 256, 1), (64, 320, 1), (64, 320, 3), (64, 576, 1))


def _blk(D):
    return 16 if D == 128 else 32


def _decode_starts(D, c):
    """starts of {0, 1, 15, 16, 17, 31, 32, 33, counter}; the counter itself (real length 1), exactly one block and one block plus
    one row (the new token at row c included)"""
    return ((0, 1, c), (15, 16, 17), (31, 32, 33), (c + 1 - _blk(D), c - _blk(D), 0))


def _sentinel_(x, b, lo, hi):
    _bits_view(x)[b, :, lo:hi] = np.int16(NAN_BITS)


def _bits_view(x):
    return x.view(torch.int16)


def _decode_inputs(D, S, seed):
    rng = np.random.default_rng(seed)
    c = ac.random_case(B_DEC, H, HKV, S, D, seed)
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    return dict(q=t(c["q"]), kc=t(c["k"]), vc=t(c["v"]), k_new=t(ac.normal_f16(rng, (B_DEC, HKV, D))),
                v_new=t(ac.nonzero_normal_f16(rng, (B_DEC, HKV, D))), table=t(ac.rope_table(D, 1024)),
                mask=t(ac.random_mask(B_DEC, S + 8, seed + 1)), scale=c["scale"])


def _one_launch(ops, x, D, kc, vc, counter, pos, mask, splits, rows=slice(None), **kw):
    n = kc.shape[0]
    tickets = torch.zeros(n * H + 1, dtype=torch.int32, device=DEV)
    out = ops.rope_decode_attention(pos, x["q"][rows], x["k_new"][rows], x["v_new"][rows], x["table"], kc, vc, tickets, slots=counter,
                                    mask=mask, scaling=x["scale"], splits=splits, kv_len=counter, kv_len_bias=1, advance=counter, **kw)
    assert torch.count_nonzero(tickets) == 0, "tickets must be zero between launches"
    return out


def _two_launches(ops, x, D, kc, vc, counter, pos, mask, splits, rows=slice(None), **kw):
    q = x["q"][rows].clone()
    ops.rotary_embedding_neox_kvcache(pos, q, x["k_new"][rows].clone(), x["v_new"][rows], D, x["table"], kc, vc, slots=counter)
    return ops.decode_attention(q, kc, vc, mask=mask, scaling=x["scale"], splits=splits, kv_len=counter, kv_len_bias=1,
                                advance=counter, **kw)


def _padded_and_reference(ops, form, x, D, S, splits, c, starts, with_mask):
    """The padded entry on the batch (sentinel rows below every start and beyond the slot) and, per row, the existing entry on the
    row alone with its cache, counter and mask moved by the start.  Returns (out [B, H, D], caches after the call)."""
    kc, vc = x["kc"].clone(), x["vc"].clone()
    for b, s in enumerate(starts):
        for t in (kc, vc):
            _sentinel_(t, b, 0, s)
            _sentinel_(t, b, c, S)
    kc0, vc0 = kc.clone(), vc.clone()
    pos = _i64([max(0, c - s) for s in starts])
    counter = _i64([c])
    mask = x["mask"] if with_mask else None
    out = form(ops, x, D, kc, vc, counter, pos, mask, splits, kv_start=_i64(starts))
    assert int(counter.item()) == c + 1, "the counter advances once"
    assert torch.isfinite(out).all(), (starts, "NaN below a start or beyond the slot reached the output")
    untouched = torch.ones(S, dtype=torch.bool, device=DEV)
    untouched[c] = False
    for new, old in ((kc, kc0), (vc, vc0)):
        assert torch.equal(_bits_view(new)[:, :, untouched], _bits_view(old)[:, :, untouched]), "only the slot's row is written"
    for b, s in enumerate(starts):
        kr = torch.empty(1, HKV, S, D, dtype=torch.float16, device=DEV)
        vr = torch.empty_like(kr)
        for t in (kr, vr):
            _bits_view(t).fill_(NAN_BITS)
        kr[0, :, :S - s], vr[0, :, :S - s] = kc0[b, :, s:], vc0[b, :, s:]
        mr = None
        if with_mask:
            mr = torch.zeros(1, x["mask"].shape[1], dtype=torch.float16, device=DEV)
            mr[0, :x["mask"].shape[1] - s] = x["mask"][b, s:]
        cr = _i64([c - s])
        want = form(ops, x, D, kr, vr, cr, pos[b:b + 1], mr, splits, rows=slice(b, b + 1))
        where = (form.__name__, starts, b, with_mask)
        assert int(cr.item()) == c - s + 1
        assert torch.equal(_bits(out[b]), _bits(want[0])), where
        # the new row sits at the absolute slot and is the row the reference wrote at slot - s
        assert torch.equal(_bits_view(kc)[b, :, c], _bits_view(kr)[0, :, c - s]), where
        assert torch.equal(_bits_view(vc)[b, :, c], _bits_view(vr)[0, :, c - s]), where
        assert torch.equal(_bits(vc[b, :, c]), _bits(x["v_new"][b])), where
    return out, kc, vc


@pytest.mark.parametrize("with_mask", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("D,S,splits", DECODE_CASES, ids=["D%d-S%d-s%d" % c for c in DECODE_CASES])
def test_decode_rows_have_the_bits_of_the_shifted_single_row(ops, D, S, splits, with_mask):
    x = _decode_inputs(D, S, seed=S + 5 * D + splits)
    for c in (40, S - 2):
        for starts in _decode_starts(D, c):
            a, kca, vca = _padded_and_reference(ops, _one_launch, x, D, S, splits, c, starts, with_mask)
            b, kcb, vcb = _padded_and_reference(ops, _two_launches, x, D, S, splits, c, starts, with_mask)
            assert torch.equal(_bits(a), _bits(b)), (c, starts, "the one-launch and two-launch forms must agree")
            assert torch.equal(_bits_view(kca), _bits_view(kcb)) and torch.equal(_bits_view(vca), _bits_view(vcb))


@pytest.mark.parametrize("with_mask", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("D,S,splits", DECODE_CASES, ids=["D%d-S%d-s%d" % c for c in DECODE_CASES])
def test_decode_all_starts_zero_is_the_existing_entry(ops, D, S, splits, with_mask):
    x = _decode_inputs(D, S, seed=S + 3 * D + splits)
    mask = x["mask"] if with_mask else None
    for form in (_one_launch, _two_launches):
        for c in (0, 40, S - 1):
            pos = _i64([c] * B_DEC)
            outs = []
            for kw in ({}, {"kv_start": _i64([0] * B_DEC)}):
                kc, vc, counter = x["kc"].clone(), x["vc"].clone(), _i64([c])
                outs.append((form(ops, x, D, kc, vc, counter, pos, mask, splits, **kw), kc, vc, int(counter.item())))
            (a, ka, va, na), (b, kb, vb, nb) = outs
            assert na == nb == c + 1
            assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ka), _bits(kb)) and torch.equal(_bits(va), _bits(vb))


@pytest.mark.parametrize("D,S,splits", DECODE_CASES[:2] + DECODE_CASES[3:5], ids=["D%d-S%d-s%d" % c for c in DECODE_CASES[:2] + DECODE_CASES[3:5]])
def test_decode_start_beyond_the_slot_attends_the_new_token_alone(ops, D, S, splits):
    """A caller error that must stay in range: the row attends its new token alone (the answer is the new value row, bit for bit)
    and nothing but the slot's row is written."""
    x = _decode_inputs(D, S, seed=S + D + splits)
    c = 40
    starts = (c + 1, S - 1, S + 100)
    for form in (_one_launch, _two_launches):
        kc, vc = x["kc"].clone(), x["vc"].clone()
        for t in (kc, vc):
            for b in range(B_DEC):
                _sentinel_(t, b, 0, c)
                _sentinel_(t, b, c, S)
        kc0, vc0 = kc.clone(), vc.clone()
        counter = _i64([c])
        out = form(ops, x, D, kc, vc, counter, _i64([0] * B_DEC), None, splits, kv_start=_i64(starts))
        assert int(counter.item()) == c + 1 and torch.isfinite(out).all()
        want = x["v_new"].repeat_interleave(H // HKV, dim=1)
        assert torch.equal(_bits(out), _bits(want)), form.__name__
        untouched = torch.ones(S, dtype=torch.bool, device=DEV)
        untouched[c] = False
        assert torch.equal(_bits_view(kc)[:, :, untouched], _bits_view(kc0)[:, :, untouched])
        assert torch.equal(_bits_view(vc)[:, :, untouched], _bits_view(vc0)[:, :, untouched])


def test_decode_kv_start_is_checked(ops):
    x = _decode_inputs(64, 64, seed=2)
    for bad in (torch.zeros(B_DEC, dtype=torch.int32, device=DEV), torch.zeros(B_DEC + 1, dtype=torch.int64, device=DEV),
                torch.zeros(B_DEC, dtype=torch.int64), torch.zeros(2 * B_DEC, dtype=torch.int64, device=DEV)[::2]):
        with pytest.raises(RuntimeError, match="kv_start"):
            ops.decode_attention(x["q"], x["kc"], x["vc"], kv_start=bad)
        with pytest.raises(RuntimeError, match="kv_start"):
            _one_launch(ops, x, 64, x["kc"], x["vc"], _i64([3]), _i64([3] * B_DEC), None, 1, kv_start=bad)
