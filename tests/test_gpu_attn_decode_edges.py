"""Decode attention (eetq_amd/csrc/attn_decode.hip) at the shapes where its paths change, with inputs on which ONE lost,
doubled or shifted cache row shows: the three families of tests/attn_cases.py against its float64 reference.

  hot row  out == V[r] BIT FOR BIT, r swept over every valid position (a different r in every (b, h) of a launch)
  census   out within 1 fp16 ulp of the float64 mean
  random   |out - ref| < 2e-3, the bound of the existing decode-attention tests, with an aperiodic finite / -inf mask

The table below names the smallest shapes that reach each path; the coverage guard restates the three launch-time
decisions of the kernel file (long_chunks, the merge's JN, its 64-record blocks) and fails when a row no longer reaches what
it claims.  The guard is never a source of expected values."""
import functools

import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-3   # the project's bound for decode attention on N(0, 1) data (test_gpu_parity.py, test_gpu_decode_step.py)


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


# ---- the kernel's launch-time decisions, restated (guard only) ---------------------------------------------------------------
K_UA, K_UB, K_UL = 8, 8, 4          # blocks requested up front (A, B) and per further trip of a LONG launch
K_UG_BLOCKS = 4                     # blocks per trip inside A and B


def blk(D):
    """rows per block: four waves of 64 / (D / 8) positions"""
    return 4 * (64 // (D // 8))


def nblocks(D, rows):
    return -(-rows // blk(D))


def long_chunks(D, S, splits):
    return -(-nblocks(D, S) // splits) > K_UA + K_UB


def merge_jn(D, splits):
    """JN of every 64-record block of the merge"""
    ns = 4 * (64 // (D // 4))
    out = []
    for s0 in range(0, splits, 64):
        j = -(-min(64, splits - s0) // ns)
        out.append(j if j <= 4 else -(-64 // ns))
    return out


def merge_blocks(splits):
    return -(-splits // 64)


def long_trips(D, sv, split, splits):
    """blocks below the valid length in each trip of the LONG loop of chunk `split`"""
    nb, ub, trips = nblocks(D, sv), K_UA + K_UB, []
    while split + ub * splits < nb:
        trips.append(sum(1 for u in range(K_UL) if split + (ub + u) * splits < nb))
        ub += K_UL
    return trips


SV_SWEEP = (0, 1, 16, 17, 255, 256, 257, 512, 513, 700)
SPLITS_SWEEP = (8, 9, 16, 17, 24, 25, 32, 33, 64, 65, 130)

# row -> (D, S, splits) cases
ROWS = {
    1: [(128, 700, 2)],                                            # LONG, stride 2, two `while` trips, ragged last trip
    2: [(128, 1000, 3)],                                           # LONG, stride 3
    3: [(128, 272, 1), (128, 256, 1), (128, 257, 1)],              # 17 blocks: just LONG; 16: just not; one row past 16
    4: [(64, 1200, 2), (64, 1500, 2)],                             # LONG at D = 64, stride 2
    5: [(64, 512, 1), (64, 513, 1), (64, 544, 1)],                 # the LONG boundary at BLK = 32
    6: [(D, 1040, s) for D in (128, 64) for s in SPLITS_SWEEP],    # every JN for both NS; 1, 2, 3 merge blocks
    7: [(128, 700, 2)],                                            # kv_len on the device: SV_SWEEP (a LONG launch, few rows)
    8: [(64, 96, 33)],                                             # more chunks than blocks: empty records in the merge
}


def check_coverage():
    """Every row of the table reaches what its comment claims."""
    assert blk(128) == 16 and blk(64) == 32
    (D, S, sp), = ROWS[1]
    assert long_chunks(D, S, sp) and sp == 2
    assert any(len(t) == 2 and t[-1] < K_UL for t in (long_trips(D, S, c, sp) for c in range(sp))), "two trips, ragged last"
    (D, S, sp), = ROWS[2]
    assert long_chunks(D, S, sp) and sp == 3 and all(len(long_trips(D, S, c, sp)) >= 2 for c in range(sp))
    assert [(nblocks(D, S), long_chunks(D, S, sp)) for D, S, sp in ROWS[3]] == [(17, True), (16, False), (17, True)]
    assert all(D == 64 and sp == 2 and long_chunks(D, S, sp) and len(long_trips(D, S, 0, sp)) >= 1 for D, S, sp in ROWS[4])
    assert [(nblocks(D, S), long_chunks(D, S, sp)) for D, S, sp in ROWS[5]] == [(16, False), (17, True), (17, True)]
    for D, jns in ((128, {1, 2, 3, 4, 8}), (64, {1, 2, 3, 4})):
        mine = [c for c in ROWS[6] if c[0] == D]
        assert {j for _, _, sp in mine for j in merge_jn(D, sp)} == jns, "every JN of this NS"
        assert {merge_blocks(sp) for _, _, sp in mine} == {1, 2, 3}
        assert not any(long_chunks(*c) for c in mine)
    # a chunk whose record index is >= 64 owns valid rows (D = 128: 65 blocks; at D = 64 there are 33, records >= 33 are empty)
    assert any(D == 128 and sp > 64 and nblocks(D, S) > 64 for D, S, sp in ROWS[6])
    (D, S, sp), = ROWS[7]
    assert long_chunks(D, S, sp) and SV_SWEEP[-1] == S and SV_SWEEP[0] == 0
    (D, S, sp), = ROWS[8]
    assert sp > nblocks(D, S) and sp <= S
    for cases in ROWS.values():
        for D, S, sp in cases:
            assert S <= 1600 and 1 <= sp <= S


def test_coverage_guard():
    check_coverage()


def _ids(cases):
    return ["D%d-S%d-x%d" % c for c in cases]


ALL = [c for r in (1, 2, 3, 4, 5, 6, 8) for c in ROWS[r]]
ALL_FAMILIES = [c for r in (1, 2, 5) for c in ROWS[r]]
ROW7 = [ROWS[7][0] + (sv,) for sv in SV_SWEEP]
ROW7_IDS = ["D%d-S%d-x%d-Sv%d" % c for c in ROW7]
STRIDED = ROWS[1] + ROWS[5]
ONE_LAUNCH = ROWS[1] + ROWS[5] + [c for c in ROWS[6] if c[2] in (17, 65)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _len(sv):
    return None if sv is None else torch.tensor(sv, dtype=torch.int64, device=DEV)


def _bits_differ(out, exp):
    """per (b, h): any channel whose bits differ"""
    D = out.shape[-1]
    return (out.reshape(-1, D).view(torch.int16) != exp.reshape(-1, D).view(torch.int16)).any(-1)


def _where(D, splits, r):
    b = r // blk(D)
    return "row %d = block %d, chunk %d, %s" % (r, b, b % splits, "trip A/B" if b // splits < K_UA + K_UB
                                                else "LONG trip %d" % ((b // splits - K_UA - K_UB) // K_UL))


def _report(D, splits, fails):
    """fails: [(r tensor [n], bad tensor [n])] -> assertion with the first few failing positions"""
    r = torch.cat([f[0] for f in fails]).cpu().numpy()
    bad = torch.cat([f[1] for f in fails]).cpu().numpy()
    assert not bad.any(), "%d of %d hot rows are not returned bit for bit; first: %s" % (
        bad.sum(), bad.size, "; ".join(_where(D, splits, int(x)) for x in r[bad][:6]))


# ---- hot row ---------------------------------------------------------------------------------------------------------------
HOT_B, HOT_H = 2, 32


@functools.lru_cache(maxsize=1)
def _hot_case(D, S, B=HOT_B, H=HOT_H):
    c = ac.hot_base(B, H, S, D, seed=1000 * D + S)
    return {n: (_t(x) if isinstance(x, np.ndarray) else x) for n, x in c.items()}


def _pairs(B, H):
    return (torch.arange(B, device=DEV).repeat_interleave(H), torch.arange(H, device=DEV).repeat(B))


def _hot_sweep(ops, D, S, splits, q, k, v, hot, scale, sv=None):
    """k is edited in place and restored"""
    B, H = q.shape[:2]
    n_valid = S if sv is None else sv
    ib, ih = _pairs(B, H)
    fails = []
    for launch in range(ac.sweep_launches(n_valid, B * H)):
        r = _t(ac.sweep(n_valid, B * H, launch))
        saved = k[ib, ih, r].clone()
        k[ib, ih, r] = hot.reshape(B * H, D)
        out = ops.decode_attention(q, k, v, scaling=scale, splits=splits, kv_len=_len(sv))
        k[ib, ih, r] = saved
        fails.append((r, _bits_differ(out, v[ib, ih, r])))
    _report(D, splits, fails)


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_hot_row_every_position(ops, D, S, splits):
    """The hot key at every position of the cache in turn, 64 positions per launch: out == V[r] bit for bit."""
    c = _hot_case(D, S)
    _hot_sweep(ops, D, S, splits, c["q"], c["k"], c["v"], c["hot"], c["scale"])


@pytest.mark.parametrize("D,S,splits,sv", ROW7, ids=ROW7_IDS)
def test_hot_row_every_valid_position_under_kv_len(ops, D, S, splits, sv):
    """Row 7: a LONG launch whose valid length comes from the device; Sv = 0 gives zeros."""
    c = _hot_case(D, S)
    if sv == 0:
        out = ops.decode_attention(c["q"], c["k"], c["v"], scaling=c["scale"], splits=splits, kv_len=_len(0))
        assert torch.count_nonzero(out) == 0 and not torch.isnan(out).any()
        return
    _hot_sweep(ops, D, S, splits, c["q"], c["k"], c["v"], c["hot"], c["scale"], sv=sv)


def _edge_rows(D, S, splits, limit, n, seed):
    """n rows below `limit`, distinct while limit >= n: the rows around the blocks where a trip form ends, then random ones"""
    b = blk(D)
    rows = [0, limit - 1, limit // 2]
    for first in (1, splits, K_UG_BLOCKS * splits, K_UA * splits, (K_UA + K_UB) * splits, (K_UA + K_UB + K_UL) * splits,
                  nblocks(D, limit) - 1):
        rows += [first * b - 1, first * b, first * b + 1]
    rows = list(dict.fromkeys(x for x in rows if 0 <= x < limit))[:n]
    taken = set(rows)
    rest = [int(x) for x in np.random.default_rng(seed).permutation(limit) if int(x) not in taken]
    return np.resize(np.array(rows + rest[: n - len(rows)], dtype=np.int64), n)


VAR_B, VAR_H, MASK_PAD = 16, 4, 40


@functools.lru_cache(maxsize=1)
def _var_case(D, S):
    return _hot_case.__wrapped__(D, S, VAR_B, VAR_H)


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_hot_row_past_the_valid_length(ops, D, S, splits):
    """A hotter key at row Sv, the first invalid one, with a sentinel V: the answer is the hot row among the valid ones.  Sv
    ragged and Sv a whole number of blocks."""
    c = _var_case(D, S)
    B, H = VAR_B, VAR_H
    ib, ih = _pairs(B, H)
    for sv in (S - blk(D) - 5, (nblocks(D, S) // 2) * blk(D)):
        k, v = c["k"].clone(), c["v"].clone()
        k[:, :, sv] = c["hotter"]
        v[:, :, sv] = 777.0
        r = _t(_edge_rows(D, S, splits, sv, B * H, seed=sv))
        k[ib, ih, r] = c["hot"].reshape(B * H, D)
        out = ops.decode_attention(c["q"], k, v, scaling=c["scale"], splits=splits, kv_len=_len(sv))
        _report(D, splits, [(r, _bits_differ(out, v[ib, ih, r]))])


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_hot_row_by_mask_alone(ops, D, S, splits):
    """K = 0: the scores are the mask.  mask[b, r_b] = 0, every other element -200 (finite in fp16), rows S + 40 long: pins the
    mask element to its position and the batch stride."""
    c = _var_case(D, S)
    B, H = VAR_B, VAR_H
    k = torch.zeros_like(c["k"])
    rows = _edge_rows(D, S, splits, S, 2 * B, seed=S + splits)
    fails = []
    for r in (_t(rows[:B]), _t(rows[B:])):
        mask = torch.full((B, S + MASK_PAD), -200.0, dtype=torch.float16, device=DEV)
        mask[:, S:] = 0.0   # never read: beyond the cache
        mask[torch.arange(B, device=DEV), r] = 0.0
        out = ops.decode_attention(c["q"], k, c["v"], mask=mask, scaling=c["scale"], splits=splits)
        exp = c["v"][torch.arange(B, device=DEV), :, r]
        fails.append((r.repeat_interleave(H), _bits_differ(out, exp)))
    _report(D, splits, fails)


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_masked_hot_row(ops, D, S, splits):
    """A hotter key at r1 under mask -inf: the answer is the second hot row -- one row after r1, one block after, half a
    cache away, one row before (head by head)."""
    c = _var_case(D, S)
    B, H = VAR_B, VAR_H
    ib, ih = _pairs(B, H)
    r1 = _t(_edge_rows(D, S, splits, S, B, seed=7 * S + splits))
    off = torch.tensor([1, blk(D), S // 2 + 3, S - 1], device=DEV)
    r2 = (r1[:, None] + off[None, :]).flatten() % S
    k = c["k"].clone()
    k[torch.arange(B, device=DEV), :, r1] = c["hotter"]
    k[ib, ih, r2] = c["hot"].reshape(B * H, D)
    mask = torch.zeros((B, S + MASK_PAD), dtype=torch.float16, device=DEV)
    mask[torch.arange(B, device=DEV), r1] = float("-inf")
    out = ops.decode_attention(c["q"], k, c["v"], mask=mask, scaling=c["scale"], splits=splits)
    _report(D, splits, [(r2, _bits_differ(out, c["v"][ib, ih, r2]))])


@pytest.mark.parametrize("D,S,splits", STRIDED, ids=_ids(STRIDED))
def test_hot_row_strided_layouts(ops, D, S, splits):
    """The sweep again with (a) K a permuted view of [B, S, H, D] storage (row stride H D, head stride D), V rows padded to
    D + 8; (b) the two layouts exchanged; the query a slice of a wider fused row in both."""
    c = _hot_case(D, S)
    B, H = HOT_B, HOT_H
    fused = torch.full((B, 8 + H * D + 24), 9.0, dtype=torch.float16, device=DEV)
    fused[:, 8: 8 + H * D] = c["q"].reshape(B, H * D)
    q = fused[:, 8: 8 + H * D].unflatten(-1, (H, D))

    def permuted(x):
        return torch.empty((B, S, H, D), dtype=torch.float16, device=DEV).permute(0, 2, 1, 3).copy_(x)

    def padded(x):
        return torch.full((B, H, S, D + 8), 5.0, dtype=torch.float16, device=DEV)[..., :D].copy_(x)

    for lay_k, lay_v in ((permuted, padded), (padded, permuted)):
        k, v = lay_k(c["k"]), lay_v(c["v"])
        assert k.stride() != v.stride() and not k.is_contiguous() and not v.is_contiguous() and q.stride(0) != H * D
        _hot_sweep(ops, D, S, splits, q, k, v, c["hot"], c["scale"])


# ---- census ----------------------------------------------------------------------------------------------------------------
CEN_B, CEN_H, CEN_HKV = 2, 16, 4


def _census(ops, D, S, splits, sv):
    """q = 0 and integer V: every weight is 1, l = Sv and sum V are exact in fp32, so the kernel's only roundings are the
    final fp32 division (relative error 2^-24, a 2^-13 part of an fp16 ulp) and the rounding of that quotient to fp16 (half
    an ulp): the result must lie within ONE fp16 ulp of the float64 mean.  A row dropped or counted twice moves it by more
    than 3 (test_attn_cases_cpu.py)."""
    v, k = ac.census_values(CEN_B, CEN_HKV, S, D, seed=D + S)
    q = torch.zeros((CEN_B, CEN_H, D), dtype=torch.float16, device=DEV)
    out = ops.decode_attention(q, _t(k), _t(v), scaling=D ** -0.5, splits=splits, kv_len=_len(sv))
    n = S if sv is None else sv
    ref = ac.reference(q.cpu().numpy(), k, v, n, D ** -0.5)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref) / ac.fp16_ulp(ref)
    print("attn-edges census D=%d S=%d splits=%d Sv=%d: max error %.3f ulp" % (D, S, splits, n, err.max()))
    assert np.isfinite(err).all() and err.max() <= 1.0


@pytest.mark.parametrize("D,S,splits", ALL_FAMILIES, ids=_ids(ALL_FAMILIES))
def test_census(ops, D, S, splits):
    """Within 1 fp16 ulp of the float64 mean: one fp32 division error, then one rounding to fp16 (see _census)."""
    _census(ops, D, S, splits, None)


@pytest.mark.parametrize("D,S,splits,sv", ROW7, ids=ROW7_IDS)
def test_census_under_kv_len(ops, D, S, splits, sv):
    """Row 7, same bound of 1 fp16 ulp (see _census); Sv = 0 gives zeros."""
    _census(ops, D, S, splits, sv)


# ---- random, finite masks --------------------------------------------------------------------------------------------------
RND_B, RND_H, RND_HKV, RND_PAD = 2, 8, 2, 24


def _random(ops, D, S, splits, sv):
    c = ac.random_case(RND_B, RND_H, RND_HKV, S, D, seed=3 * S + D)
    mask = ac.random_mask(RND_B, S + RND_PAD, seed=S + D + splits)
    out = ops.decode_attention(_t(c["q"]), _t(c["k"]), _t(c["v"]), mask=_t(mask), scaling=c["scale"], splits=splits,
                               kv_len=_len(sv))
    n = S if sv is None else sv
    ref = ac.reference(c["q"], c["k"], c["v"], n, c["scale"], mask)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print("attn-edges random D=%d S=%d splits=%d Sv=%d: max |out - ref| %.3e" % (D, S, splits, n, err))
    assert torch.isfinite(out).all() and err < TOL
    if n == 0:
        assert torch.count_nonzero(out) == 0


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_random_with_finite_masks(ops, D, S, splits):
    _random(ops, D, S, splits, None)


@pytest.mark.parametrize("D,S,splits,sv", ROW7, ids=ROW7_IDS)
def test_random_with_finite_masks_under_kv_len(ops, D, S, splits, sv):
    _random(ops, D, S, splits, sv)


# ---- one launch against two ------------------------------------------------------------------------------------------------
def _slots(D, S, splits):
    """row 0, a block's last row, a block's first row, the first row owned by a LONG trip (where there is one), S - 1"""
    rows = [0, blk(D) - 1, blk(D), (K_UA + K_UB) * splits * blk(D), S - 1]
    return [r for r in dict.fromkeys(rows) if r < S]


def _both_forms(ops, D, S, splits, q, k_new, v_new, pos, table, kc, vc, slot, mask, scale):
    """The new token at row `slot` of a full cache (the counter stands at S - 1), by the two-launch pair on one copy of the
    caches and by the one-launch form on another: (out, rotated q, caches) of the one-launch form after the three checks."""
    B, H = q.shape[:2]
    kc_a, vc_a, kc_b, vc_b = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    cnt_a = torch.tensor(S - 1, dtype=torch.int64, device=DEV)
    cnt_b = cnt_a.clone()
    slots = torch.full((B,), slot, dtype=torch.int64, device=DEV)
    tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)
    q_a = q.clone()
    ops.rotary_embedding_neox_kvcache(pos, q_a, k_new.clone(), v_new, D, table, kc_a, vc_a, slots=slots)
    out_a = ops.decode_attention(q_a, kc_a, vc_a, mask=mask, scaling=scale, splits=splits, kv_len=cnt_a, kv_len_bias=1,
                                 advance=cnt_a)
    out_b = ops.rope_decode_attention(pos, q, k_new, v_new, table, kc_b, vc_b, tickets, slots=slots, mask=mask, scaling=scale,
                                      splits=splits, kv_len=cnt_b, kv_len_bias=1, advance=cnt_b)
    where = (slot, mask is not None)
    assert torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)), where
    assert torch.equal(kc_a.view(torch.int16), kc_b.view(torch.int16)) and torch.equal(vc_a.view(torch.int16),
                                                                                      vc_b.view(torch.int16)), where
    assert not torch.equal(kc_b[:, :, slot], kc[:, :, slot]), "the new row was written"
    assert torch.count_nonzero(tickets) == 0, "tickets must be zero between launches"
    assert int(cnt_a.item()) == int(cnt_b.item()) == S, "the counter has advanced"
    return out_b, q_a, kc_b, vc_b


@pytest.mark.parametrize("D,S,splits", ONE_LAUNCH, ids=_ids(ONE_LAUNCH))
def test_one_launch_equals_two_launches_at_the_edges(ops, D, S, splits):
    """Grouped-query heads (H = 4 Hkv), the new token's row swept over the places where the substitution from registers can
    go wrong, with and without a mask: bit-identical outputs and caches, zero tickets, an advanced counter, and the float64
    reference within the project's bound."""
    B, H, Hkv = 2, 16, 4
    rng = np.random.default_rng(S + splits)
    c = ac.random_case(B, H, Hkv, S, D, seed=5 * S + D)
    q, kc, vc = _t(c["q"]), _t(c["k"]), _t(c["v"])
    k_new, v_new = _t(ac.normal_f16(rng, (B, Hkv, D))), _t(ac.normal_f16(rng, (B, Hkv, D)))
    table = _t(ac.rope_table(D, 2048))
    pos = _t(rng.integers(1, 2048, size=B).astype(np.int64))
    mask_np = ac.random_mask(B, S + RND_PAD, seed=S + 2 * splits)
    for slot in _slots(D, S, splits):
        for m in (None, mask_np):
            out, q_rot, kc_b, vc_b = _both_forms(ops, D, S, splits, q, k_new, v_new, pos, table, kc, vc, slot,
                                                 None if m is None else _t(m), c["scale"])
            ref = ac.reference(q_rot.cpu().numpy(), kc_b.cpu().numpy(), vc_b.cpu().numpy(), S, c["scale"], m)
            err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
            assert torch.isfinite(out).all() and err < TOL, (slot, m is not None, err)


@pytest.mark.parametrize("D,S,splits", ONE_LAUNCH, ids=_ids(ONE_LAUNCH))
def test_new_token_is_the_hot_row(ops, D, S, splits):
    """The hot row is the token of this step: it reaches the softmax from registers, never from the cache, in every workgroup
    of its head.  out == v_new bit for bit, in both forms."""
    B, H = 2, 16
    c = {n: (_t(x) if isinstance(x, np.ndarray) else x) for n, x in ac.new_token_hot(B, H, S, D, seed=S + D + splits).items()}
    for slot in _slots(D, S, splits):
        out, _, _, vc_b = _both_forms(ops, D, S, splits, c["q"], c["k_new"], c["v_new"], c["pos"], c["table"], c["kc"], c["vc"],
                                      slot, None, c["scale"])
        assert torch.equal(vc_b[:, :, slot].view(torch.int16), c["v_new"].view(torch.int16))
        bad = _bits_differ(out, c["v_new"])
        assert not bad.any(), "new token at %s: %d of %d heads do not return v_new bit for bit" % (
            _where(D, splits, slot), int(bad.sum()), bad.numel())
