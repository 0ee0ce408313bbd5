"""The int8 KV cache's kernels (eetq_amd/csrc/attn_decode.hip, the quantising write of norm_rope.hip) at the shapes where
the chunk code's paths change (the rows of test_gpu_attn_decode_edges.py), with the input families of tests/attn_cases.py
built as int8 bytes and fp16 scales by the NumPy quantiser of tests/kv8_cases.py:

  hot row   out == fp16(vs[r] * v8[r]) BIT FOR BIT, r swept over every valid position
  by scale  the hot row's neighbours carry its bytes with an eighth of its K scale: a row paired with a neighbour's scale fails
  census    q = 0, integer bytes, V scales cycling 0.5, 1, 2: within 1 fp16 ulp of the float64 mean
  random    |out - reference on the dequantised float64 rows| < 2e-3, the project's bound for the fp16 kernel (the kernel
            attends exactly these values, so the error budget is the same)
  write     bytes and scales of the quantising cache write bit-exact against NumPy

B = 2, H = 4, Hkv = 2 (grouped-query) unless said otherwise; the hot-row families give every head its own rows (Hkv = H), as
attn_cases.hot_base builds them."""
import functools

import numpy as np
import pytest
import torch

import attn_cases as ac
import kv8_cases as k8c

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-3
B, H, HKV = 2, 4, 2
PAD = 24

LONG = [(128, 700, 2), (64, 1200, 2)]
BOUNDARY = [(128, 256, 1), (128, 272, 1), (64, 512, 1), (64, 544, 1)]
MERGE = [(128, 1040, 17), (64, 1040, 65)]
MANY_CHUNKS = [(64, 96, 33)]
ALL = LONG + BOUNDARY + MERGE + MANY_CHUNKS
SV_SWEEP = (0, 1, 16, 17, 255, 256, 257, 512, 513, 700)
UNDER_LEN = [(128, 700, 2, sv) for sv in SV_SWEEP]
STRIDED = [(128, 700, 2), (64, 544, 1)]
# the fp16 test's ONE_LAUNCH shapes: LONG, the LONG boundary at D = 64, merge widths 17 and 65 at both head sizes
ONE_LAUNCH = [(128, 700, 2), (64, 512, 1), (64, 513, 1), (64, 544, 1), (128, 1040, 17), (128, 1040, 65), (64, 1040, 17),
              (64, 1040, 65)]


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


def blk(D):
    return 4 * (64 // (D // 8))


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _len(sv):
    return None if sv is None else torch.tensor(sv, dtype=torch.int64, device=DEV)


def _bits_differ(out, exp):
    D = out.shape[-1]
    return (out.reshape(-1, D).view(torch.int16) != exp.reshape(-1, D).view(torch.int16)).any(-1)


def _pairs(nb, nh):
    return (torch.arange(nb, device=DEV).repeat_interleave(nh), torch.arange(nh, device=DEV).repeat(nb))


def _report(D, fails):
    r = torch.cat([f[0] for f in fails]).cpu().numpy()
    bad = torch.cat([f[1] for f in fails]).cpu().numpy()
    assert not bad.any(), "%d of %d hot rows are not returned bit for bit; first rows: %s (block size %d)" % (
        bad.sum(), bad.size, r[bad][:8].tolist(), blk(D))


# ---- hot row ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _hot_case(D, S):
    c = ac.hot_base(B, H, S, D, seed=1000 * D + S)      # every head its own rows: k, v [B, H, S, D]
    qc = k8c.quantize_cache(c["k"], c["v"])
    hot8, hots = k8c.quantize_rows(c["hot"])
    hotter8, hotters = k8c.quantize_rows(c["hotter"])
    gap = ac.hot_gap(c["q"], qc["kd"], k8c.dequantize_rows(hot8, hots), c["scale"])
    # the decoys of the by-scale family: the hotter key's bytes under an eighth of its scale, against the hotter key itself
    eighth = (hotters.astype(np.float32) / np.float32(8)).astype(np.float16)
    assert np.array_equal(eighth.astype(np.float64) * 8, hotters.astype(np.float64)), "an eighth of the scale is exact"
    q64 = c["q"].astype(np.float64)
    s_hotter = (q64 * k8c.dequantize_rows(hotter8, hotters)).sum(-1) * c["scale"]
    s_decoy = (q64 * k8c.dequantize_rows(hotter8, eighth)).sum(-1) * c["scale"]
    gap_scale = float((s_hotter - np.maximum(s_decoy, ac.scores(c["q"], qc["kd"], c["scale"]).max(-1))).min())
    print("kv8 hot case D=%d S=%d: quantised hot key gap %.1f, hotter against its decoys %.1f" % (D, S, gap, gap_scale))
    return dict(q=_t(c["q"]), k8=_t(qc["k8"]), v8=_t(qc["v8"]), sc=_t(qc["scales"]), exp=_t(k8c.hot_value(qc["v8"], qc["scales"][..., 1])),
                hot8=_t(hot8), hots=_t(hots), hotter8=_t(hotter8), hotters=_t(hotters), eighth=_t(eighth), scale=c["scale"],
                gap=gap, gap_scale=gap_scale)


def _hot_sweep(ops, D, S, splits, c, sv=None, views=None):
    """the cache is edited in place and restored"""
    k8, v8, sc = views if views is not None else (c["k8"], c["v8"], c["sc"])
    n_valid = S if sv is None else sv
    ib, ih = _pairs(B, H)
    fails = []
    for launch in range(ac.sweep_launches(n_valid, B * H)):
        r = _t(ac.sweep(n_valid, B * H, launch))
        saved8, saveds = k8[ib, ih, r].clone(), sc[ib, ih, r, 0].clone()
        k8[ib, ih, r] = c["hot8"].reshape(B * H, D)
        sc[ib, ih, r, 0] = c["hots"].reshape(B * H)
        out = ops.decode_attention_i8kv(c["q"], k8, v8, sc, scaling=c["scale"], splits=splits, kv_len=_len(sv))
        k8[ib, ih, r] = saved8
        sc[ib, ih, r, 0] = saveds
        fails.append((r, _bits_differ(out, c["exp"][ib, ih, r])))
    _report(D, fails)


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_hot_row_every_position(ops, D, S, splits):
    """The quantised hot key at every position in turn: out == fp16(vs[r] * v8[r]) bit for bit."""
    c = _hot_case(D, S)
    assert c["gap"] >= ac.GAP_MIN
    _hot_sweep(ops, D, S, splits, c)


@pytest.mark.parametrize("D,S,splits,sv", UNDER_LEN, ids=_ids(UNDER_LEN))
def test_hot_row_under_kv_len(ops, D, S, splits, sv):
    """The valid length comes from the device; Sv = 0 gives zeros."""
    c = _hot_case(D, S)
    assert c["gap"] >= ac.GAP_MIN
    if sv == 0:
        out = ops.decode_attention_i8kv(c["q"], c["k8"], c["v8"], c["sc"], scaling=c["scale"], splits=splits, kv_len=_len(0))
        assert torch.count_nonzero(out) == 0 and not torch.isnan(out).any()
        return
    _hot_sweep(ops, D, S, splits, c, sv=sv)


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_hot_by_scale_alone(ops, D, S, splits):
    """Rows r - 1 and r + 1 carry the hot row's bytes with an eighth of its K scale: the row wins by its scale alone, and a
    kernel that pairs a row with a neighbour's scale returns a neighbour's V row."""
    c = _hot_case(D, S)
    assert c["gap_scale"] >= ac.GAP_MIN
    k8, sc = c["k8"], c["sc"]
    ib, ih = _pairs(B, H)
    fails = []
    for launch in range(ac.sweep_launches(S - 2, B * H)):
        r = _t(ac.sweep(S - 2, B * H, launch)) + 1
        rows = torch.stack([r - 1, r, r + 1], dim=1)                                  # [B H, 3]
        i3b, i3h = ib[:, None].expand(-1, 3), ih[:, None].expand(-1, 3)
        saved8, saveds = k8[i3b, i3h, rows].clone(), sc[i3b, i3h, rows, 0].clone()
        k8[i3b, i3h, rows] = c["hotter8"].reshape(B * H, 1, D).expand(-1, 3, -1)
        sc[i3b, i3h, rows, 0] = torch.stack([c["eighth"].reshape(-1), c["hotters"].reshape(-1), c["eighth"].reshape(-1)], dim=1)
        out = ops.decode_attention_i8kv(c["q"], k8, c["v8"], sc, scaling=c["scale"], splits=splits)
        k8[i3b, i3h, rows] = saved8
        sc[i3b, i3h, rows, 0] = saveds
        fails.append((r, _bits_differ(out, c["exp"][ib, ih, r])))
    _report(D, fails)


@pytest.mark.parametrize("D,S,splits", STRIDED, ids=_ids(STRIDED))
def test_hot_row_strided_cache(ops, D, S, splits):
    """K a permuted view of [B, S, H, D] storage, V rows padded to D + 8 bytes, the scales a view of [B, H, S, 4] storage."""
    c = _hot_case(D, S)
    k8 = torch.empty((B, S, H, D), dtype=torch.int8, device=DEV).permute(0, 2, 1, 3).copy_(c["k8"])
    v8 = torch.full((B, H, S, D + 8), 5, dtype=torch.int8, device=DEV)[..., :D].copy_(c["v8"])
    sc = torch.full((B, H, S, 4), 9.0, dtype=torch.float16, device=DEV)[..., :2].copy_(c["sc"])
    assert not k8.is_contiguous() and not v8.is_contiguous() and not sc.is_contiguous() and k8.stride() != v8.stride()
    _hot_sweep(ops, D, S, splits, c, views=(k8, v8, sc))


# ---- census ----------------------------------------------------------------------------------------------------------------
def _census(ops, D, S, splits, sv):
    vint, k = ac.census_values(B, HKV, S, D, seed=D + S)
    v8 = vint.astype(np.int8)
    vs = np.broadcast_to(k8c.census_scales(S), (B, HKV, S))
    k8, ks = k8c.quantize_rows(k)
    vd = k8c.dequantize_rows(v8, vs)
    n = S if sv is None else sv
    q = np.zeros((B, H, D), dtype=np.float16)
    out = ops.decode_attention_i8kv(_t(q), _t(k8), _t(v8), _t(k8c.scale_pairs(ks, vs)), scaling=D ** -0.5, splits=splits,
                                    kv_len=_len(sv))
    if n == 0:
        assert torch.count_nonzero(out) == 0 and not torch.isnan(out).any()
        return
    # a dropped or doubled row must move the mean by more than the tolerance (1 ulp) and the kernel's own error (< 1 ulp)
    drop, dbl = ac.census_shift_ulps(vd, n)
    assert drop > 3 and (dbl is None or dbl > 3), (drop, dbl)
    ref = ac.reference(q, k8c.dequantize_rows(k8, ks), vd, n, D ** -0.5)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref) / ac.fp16_ulp(ref)
    print("kv8 census D=%d S=%d splits=%d Sv=%d: max error %.3f ulp, a row shifts the mean by >= %.0f ulp" % (
        D, S, splits, n, err.max(), drop if dbl is None else min(drop, dbl)))
    assert np.isfinite(err).all() and err.max() <= 1.0


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_census(ops, D, S, splits):
    """Every weight is 1, l = Sv and the sum of vs * v8 are exact in fp32: one fp32 division and one rounding to fp16 remain."""
    _census(ops, D, S, splits, None)


@pytest.mark.parametrize("D,S,splits,sv", UNDER_LEN, ids=_ids(UNDER_LEN))
def test_census_under_kv_len(ops, D, S, splits, sv):
    _census(ops, D, S, splits, sv)


# ---- random, finite masks --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _random_case(D, S):
    c = ac.random_case(B, H, HKV, S, D, seed=3 * S + D)
    return c, k8c.quantize_cache(c["k"], c["v"])


@pytest.mark.parametrize("D,S,splits", ALL, ids=_ids(ALL))
def test_random_with_finite_masks(ops, D, S, splits):
    c, qc = _random_case(D, S)
    mask = ac.random_mask(B, S + PAD, seed=S + D + splits)
    out = ops.decode_attention_i8kv(_t(c["q"]), _t(qc["k8"]), _t(qc["v8"]), _t(qc["scales"]), mask=_t(mask), scaling=c["scale"],
                                    splits=splits)
    ref = ac.reference(c["q"], qc["kd"], qc["vd"], S, c["scale"], mask)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print("kv8 random D=%d S=%d splits=%d: max |out - ref| %.3e" % (D, S, splits, err))
    assert torch.isfinite(out).all() and err < TOL


@pytest.mark.parametrize("D,S,splits", STRIDED, ids=_ids(STRIDED))
def test_random_strided_cache(ops, D, S, splits):
    """Grouped-query heads over a cache whose rows are D + 8 bytes apart, a permuted V and a scale tensor that is a view."""
    c, qc = _random_case(D, S)
    k8 = torch.full((B, HKV, S, D + 8), 5, dtype=torch.int8, device=DEV)[..., :D].copy_(_t(qc["k8"]))
    v8 = torch.empty((B, S, HKV, D), dtype=torch.int8, device=DEV).permute(0, 2, 1, 3).copy_(_t(qc["v8"]))
    sc = torch.full((B, HKV, S, 6), 9.0, dtype=torch.float16, device=DEV)[..., 2:4].copy_(_t(qc["scales"]))
    mask = ac.random_mask(B, S + PAD, seed=S + D)
    out = ops.decode_attention_i8kv(_t(c["q"]), k8, v8, sc, mask=_t(mask), scaling=c["scale"], splits=splits)
    ref = ac.reference(c["q"], qc["kd"], qc["vd"], S, c["scale"], mask)
    assert np.abs(out.cpu().numpy().astype(np.float64) - ref).max() < TOL


# ---- one launch against two ------------------------------------------------------------------------------------------------
K_UA, K_UB = 8, 8


def _slots(D, S, splits):
    rows = [0, blk(D) - 1, blk(D), (K_UA + K_UB) * splits * blk(D), S - 1]
    return [r for r in dict.fromkeys(rows) if r < S]


def _both_forms(ops, D, S, splits, q, k_new, v_new, pos, table, k8, v8, sc, slot, mask, scale):
    """The new token at row `slot` of a full cache (the counter stands at S - 1): the quantising write with one token followed
    by the two-launch attention on one copy of the cache, the one-launch form on another."""
    nb, nh = q.shape[:2]
    a, b = [x.clone() for x in (k8, v8, sc)], [x.clone() for x in (k8, v8, sc)]
    cnt_a = torch.tensor(S - 1, dtype=torch.int64, device=DEV)
    cnt_b = cnt_a.clone()
    slots = torch.full((nb,), slot, dtype=torch.int64, device=DEV)
    tickets = torch.zeros(nb * nh + 1, dtype=torch.int32, device=DEV)
    q_a, k_a = q.clone(), k_new.clone()
    ops.rotary_embedding_neox_kvcache_prefill_i8(pos[:, None].contiguous(), q_a[:, None], k_a[:, None], v_new[:, None], D, table,
                                                 a[0], a[1], a[2], first_row_dev=slots[:1])
    out_a = ops.decode_attention_i8kv(q_a, a[0], a[1], a[2], mask=mask, scaling=scale, splits=splits, kv_len=cnt_a, kv_len_bias=1,
                                      advance=cnt_a)
    out_b = ops.rope_decode_attention_i8kv(pos, q, k_new, v_new, table, b[0], b[1], b[2], tickets, slots=slots, mask=mask,
                                           scaling=scale, splits=splits, kv_len=cnt_b, kv_len_bias=1, advance=cnt_b)
    where = (slot, mask is not None)
    assert torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)), where
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int16), b[2].view(torch.int16)), where
    assert torch.count_nonzero(tickets) == 0, "tickets must be zero between launches"
    assert int(cnt_a.item()) == int(cnt_b.item()) == S, "the counter has advanced"
    # the written row: the NumPy quantiser of the NumPy rotation of k, and of v
    kr = ac.rope_neox_f16(k_new.cpu().numpy(), table.cpu().numpy(), pos.cpu().numpy())
    ek8, eks = k8c.quantize_rows(kr)
    ev8, evs = k8c.quantize_rows(v_new.cpu().numpy())
    assert np.array_equal(b[0][:, :, slot].cpu().numpy(), ek8) and np.array_equal(b[1][:, :, slot].cpu().numpy(), ev8), where
    assert np.array_equal(b[2][:, :, slot].cpu().numpy().view(np.int16), k8c.scale_pairs(eks, evs).view(np.int16)), where
    keep = torch.arange(S, device=DEV) != slot
    assert torch.equal(b[0][:, :, keep], k8[:, :, keep]) and torch.equal(b[1][:, :, keep], v8[:, :, keep]) and torch.equal(
        b[2][:, :, keep].view(torch.int16), sc[:, :, keep].view(torch.int16)), "only the new row is written"
    return out_b, q_a, b


@pytest.mark.parametrize("D,S,splits", ONE_LAUNCH, ids=_ids(ONE_LAUNCH))
def test_one_launch_equals_two_launches_at_the_edges(ops, D, S, splits):
    """Grouped-query heads, the new token's row at the places where the substitution from registers can go wrong, with and
    without a mask: bit-identical outputs, caches and scales, the written row equal to the NumPy quantiser's, zero tickets, an
    advanced counter, and the float64 reference on the dequantised rows within the project's bound."""
    rng = np.random.default_rng(S + splits)
    c, qc = _random_case(D, S)
    q, k8, v8, sc = _t(c["q"]), _t(qc["k8"]), _t(qc["v8"]), _t(qc["scales"])
    k_new, v_new = _t(ac.normal_f16(rng, (B, HKV, D))), _t(ac.normal_f16(rng, (B, HKV, D)))
    table = _t(ac.rope_table(D, 2048))
    pos = _t(rng.integers(1, 2048, size=B).astype(np.int64))
    mask_np = ac.random_mask(B, S + PAD, seed=S + 2 * splits)
    for slot in _slots(D, S, splits):
        for m in (None, mask_np):
            out, q_rot, cache = _both_forms(ops, D, S, splits, q, k_new, v_new, pos, table, k8, v8, sc, slot,
                                            None if m is None else _t(m), c["scale"])
            s_np = cache[2].cpu().numpy()
            ref = ac.reference(q_rot.cpu().numpy(), k8c.dequantize_rows(cache[0].cpu().numpy(), s_np[..., 0]),
                               k8c.dequantize_rows(cache[1].cpu().numpy(), s_np[..., 1]), S, c["scale"], m)
            err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
            assert torch.isfinite(out).all() and err < TOL, (slot, m is not None, err)


@pytest.mark.parametrize("D,S,splits", ONE_LAUNCH, ids=_ids(ONE_LAUNCH))
def test_new_token_is_the_hot_row(ops, D, S, splits):
    """The hot row is the token of this step: it reaches the softmax as its quantised self from registers, in every workgroup of
    its head.  out == fp16(vs * v8) of the new V row bit for bit, in both forms."""
    nb, nh = 2, 16
    c = ac.new_token_hot(nb, nh, S, D, seed=S + D + splits)
    qc = k8c.quantize_cache(c["kc"], c["vc"])
    qr = ac.rope_neox_f16(c["q"], c["table"], c["pos"])
    kr8, krs = k8c.quantize_rows(ac.rope_neox_f16(c["k_new"], c["table"], c["pos"]))
    assert ac.hot_gap(qr, qc["kd"], k8c.dequantize_rows(kr8, krs), c["scale"]) >= ac.GAP_MIN
    exp = _t(k8c.hot_value(*k8c.quantize_rows(c["v_new"])))
    for slot in _slots(D, S, splits):
        out, _, _ = _both_forms(ops, D, S, splits, _t(c["q"]), _t(c["k_new"]), _t(c["v_new"]), _t(c["pos"]), _t(c["table"]),
                                _t(qc["k8"]), _t(qc["v8"]), _t(qc["scales"]), slot, None, c["scale"])
        bad = _bits_differ(out, exp)
        assert not bad.any(), "new token at row %d: %d of %d heads do not return the quantised new V row" % (
            slot, int(bad.sum()), bad.numel())


@pytest.mark.parametrize("slot", [-1, 700])
def test_slot_outside_the_cache(ops, slot):
    """Neither written nor attended (and nothing is rotated), and counted: one dropped step per batch row."""
    D, S, splits = 128, 700, 2
    c, qc = _random_case(D, S)
    rng = np.random.default_rng(slot + 5)
    q, k8, v8, sc = _t(c["q"]), _t(qc["k8"]), _t(qc["v8"]), _t(qc["scales"])
    before = [x.clone() for x in (k8, v8, sc)]
    k_new, v_new = _t(ac.normal_f16(rng, (B, HKV, D))), _t(ac.normal_f16(rng, (B, HKV, D)))
    table, pos = _t(ac.rope_table(D, 2048)), _t(np.array([5, 9], dtype=np.int64))
    cnt = torch.tensor(300, dtype=torch.int64, device=DEV)
    tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)
    ops.decode_dropped_steps(reset=True)
    out = ops.rope_decode_attention_i8kv(pos, q, k_new, v_new, table, k8, v8, sc, tickets,
                                         slots=torch.full((B,), slot, dtype=torch.int64, device=DEV), scaling=c["scale"],
                                         splits=splits, kv_len=cnt, kv_len_bias=1)
    assert ops.decode_dropped_steps(reset=True) == B
    exp = ops.decode_attention_i8kv(q, k8, v8, sc, scaling=c["scale"], splits=splits, kv_len=cnt, kv_len_bias=1)
    assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
    assert torch.equal(k8, before[0]) and torch.equal(v8, before[1]) and torch.equal(sc.view(torch.int16), before[2].view(torch.int16))


# ---- the quantising cache write ----------------------------------------------------------------------------------------------
def _round_up_amax():
    """an fp16 amax whose scale fp16(amax / 127) lies ABOVE amax / 127: the largest byte of the row is then 127 after rounding
    126.9.. up, never 128"""
    for bits in range(0x3C00, 0x4400):
        a = np.array(bits, dtype=np.uint16).view(np.float16)
        s = (a.astype(np.float32) * k8c.INV127).astype(np.float16)
        if float(s) > float(a) / 127.0 * (1 + 2.0 ** -12):
            return a
    raise AssertionError("no such value")


@pytest.mark.parametrize("dev_base", [False, True], ids=["host-row", "device-row"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 5, 64])
def test_quantising_write(ops, T, D, dev_base):
    """Bytes and scales bit-exact against NumPy (an all-zero row and a row whose scale rounds up among them); q and k in the
    projection buffer equal the fp16 kernel's rotation bit for bit; rows outside the written range are untouched."""
    S, base, W = 80, 7, (H + 2 * HKV) * D
    rng = np.random.default_rng(100 * T + D)
    qkv_np = ac.normal_f16(rng, (B, T, W))
    qkv_np[0, 0, H * D: (H + 1) * D] = 0                              # K of token 0, kv head 0: all zero -> scale 0, bytes 0
    vrow = (H + HKV) * D
    qkv_np[B - 1, T - 1, vrow: vrow + D] = np.float16(0.25)           # V of the last token, kv head 0: amax as chosen
    qkv_np[B - 1, T - 1, vrow + 3] = -_round_up_amax()
    table_np = ac.rope_table(D, 2048)
    pos_np = (base + np.arange(T, dtype=np.int64))[None, :].repeat(B, 0) + np.array([[0], [11]])
    table, pos = _t(table_np), _t(pos_np)

    def views(buf):
        return (buf[..., : H * D].unflatten(-1, (H, D)), buf[..., H * D: (H + HKV) * D].unflatten(-1, (HKV, D)),
                buf[..., (H + HKV) * D:].unflatten(-1, (HKV, D)))

    qkv, qkv16 = _t(qkv_np), _t(qkv_np)
    q, k, v = views(qkv)
    k8 = torch.full((B, HKV, S, D), 0x55, dtype=torch.int8, device=DEV)
    v8 = torch.full((B, HKV, S, D), 0x33, dtype=torch.int8, device=DEV)
    sc = torch.full((B, HKV, S, 2), 7.0, dtype=torch.float16, device=DEV)
    row = dict(first_row_dev=torch.tensor(base, dtype=torch.int64, device=DEV)) if dev_base else dict(first_row=base)
    ops.rotary_embedding_neox_kvcache_prefill_i8(pos, q, k, v, D, table, k8, v8, sc, **row)
    # the fp16 kernel on a copy: the same q in place, the rotated k in its cache
    q16, k16, v16 = views(qkv16)
    kc16 = torch.zeros((B, HKV, S, D), dtype=torch.float16, device=DEV)
    vc16 = torch.zeros_like(kc16)
    ops.rotary_embedding_neox_kvcache_prefill(pos, q16, k16, v16, D, table, kc16, vc16, first_row=base)
    assert torch.equal(q.view(torch.int16), q16.view(torch.int16))
    assert torch.equal(k.transpose(1, 2).contiguous().view(torch.int16), kc16[:, :, base: base + T].contiguous().view(torch.int16))
    assert torch.equal(v.view(torch.int16), _t(qkv_np)[..., (H + HKV) * D:].unflatten(-1, (HKV, D)).view(torch.int16))
    # NumPy: rotation, then the quantiser
    k_np = qkv_np[..., H * D: (H + HKV) * D].reshape(B * T, HKV, D)
    kr = ac.rope_neox_f16(k_np, table_np, pos_np.reshape(-1)).reshape(B, T, HKV, D).transpose(0, 2, 1, 3)
    v_np = qkv_np[..., (H + HKV) * D:].reshape(B, T, HKV, D).transpose(0, 2, 1, 3)
    assert np.array_equal(kr.view(np.int16), kc16[:, :, base: base + T].cpu().numpy().view(np.int16))
    ek8, eks = k8c.quantize_rows(kr)
    ev8, evs = k8c.quantize_rows(v_np)
    assert eks[0, 0, 0] == 0 and not ek8[0, 0, 0].any() and np.abs(ev8[B - 1, 0, T - 1]).max() == 127
    assert np.array_equal(k8[:, :, base: base + T].cpu().numpy(), ek8)
    assert np.array_equal(v8[:, :, base: base + T].cpu().numpy(), ev8)
    assert np.array_equal(sc[:, :, base: base + T].cpu().numpy().view(np.int16), k8c.scale_pairs(eks, evs).view(np.int16))
    keep = torch.ones(S, dtype=torch.bool, device=DEV)
    keep[base: base + T] = False
    assert (k8[:, :, keep] == 0x55).all() and (v8[:, :, keep] == 0x33).all() and (sc[:, :, keep] == 7.0).all()


def test_quantising_write_drops_rows_outside_the_cache(ops):
    """A device base row that leaves 2 of 5 tokens inside the cache: those are written, the others dropped and counted."""
    D, S, T, W = 64, 40, 5, (H + 2 * HKV) * 64
    rng = np.random.default_rng(77)
    qkv = _t(ac.normal_f16(rng, (B, T, W)))
    q, k, v = (qkv[..., : H * D].unflatten(-1, (H, D)), qkv[..., H * D: (H + HKV) * D].unflatten(-1, (HKV, D)),
               qkv[..., (H + HKV) * D:].unflatten(-1, (HKV, D)))
    v_np = v.cpu().numpy()
    k8 = torch.full((B, HKV, S, D), 0x55, dtype=torch.int8, device=DEV)
    v8 = torch.full((B, HKV, S, D), 0x33, dtype=torch.int8, device=DEV)
    sc = torch.full((B, HKV, S, 2), 7.0, dtype=torch.float16, device=DEV)
    pos = _t(np.arange(T, dtype=np.int64)[None, :].repeat(B, 0))
    ops.decode_dropped_steps(reset=True)
    ops.rotary_embedding_neox_kvcache_prefill_i8(pos, q, k, v, D, _t(ac.rope_table(D, 64)), k8, v8, sc,
                                                 first_row_dev=torch.tensor(S - 2, dtype=torch.int64, device=DEV))
    assert ops.decode_dropped_steps(reset=True) == B * 3
    ev8, evs = k8c.quantize_rows(v_np[:, :2].transpose(0, 2, 1, 3))
    assert np.array_equal(v8[:, :, S - 2:].cpu().numpy(), ev8)
    assert np.array_equal(sc[:, :, S - 2:, 1].cpu().numpy().view(np.int16), evs.view(np.int16))
    assert (k8[:, :, : S - 2] == 0x55).all() and (v8[:, :, : S - 2] == 0x33).all() and (sc[:, :, : S - 2] == 7.0).all()
