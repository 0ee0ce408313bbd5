"""The int8 KV cache where its own tests (test_gpu_kv8_attn.py, test_gpu_kv8_decoder.py) do not look.

  edge rows   tests/kv8_cases.edge_rows through BOTH quantisers on the GPU -- the prompt writer (norm_rope.hip) and the
              in-register quantiser of the one-launch decode form (attn_decode.hip): exact ties (half away from zero, never
              to even), fp16-subnormal scales, a non-zero row whose scale rounds to 0, the clamp (it only ever bites under a
              subnormal scale), amax 65504, and a sweep that puts the row maximum on every channel in turn (the three absmax
              reductions).  Bytes and scale bit patterns equal the NumPy quantiser's.
  wide heads  33, 36, 40 and 65 KV heads: the write kernel's loops make a second and a third trip with part of a wave active.
  families    what test_gpu_attn_decode_edges.py has for the fp16 kernel and the int8 kernel lacked: a hotter key past the valid
              length (then NaN / Inf scale bit patterns and 0x7F bytes there), a hot row by mask alone, a hotter key under a -inf
              mask, random masks under kv_len, a fully masked batch row, and hot V rows with subnormal, zero and 516 scales.
  bindings    eetq_amd.ops_ctypes against the compiled module: outputs, caches, scales, counter and refusals.

Everything is compared bit for bit except the random families (|out - ref| < 2e-3 against the float64 reference on the
dequantised rows, the project's bound for this kernel family) and the rows whose V scale is 0: fp16(0 * v8) is -0 for a
negative byte in NumPy and +0 from the kernel's fused accumulate, so those compare by value.

A row whose amax is 65504 has scale 516, and its +-127 bytes dequantise to 65532, past the largest fp16 value: a query that puts
all its weight on such a row gets fp16(65532) = inf there, from NumPy and from the kernel alike.  The edge-row launches of the
one-launch form therefore pair every V row with ANOTHER row's K (V is the row list rolled by one), so that no weight is 1.

Wall time on an MI355X: 6 s for the file (78 tests), no test above 0.5 s."""
import functools

import numpy as np
import pytest
import torch

import attn_cases as ac
import kv8_cases as k8c
from test_gpu_attn_decode_edges import _edge_rows, blk, nblocks
from test_gpu_kv8_attn import (BOUNDARY, MANY_CHUNKS, MERGE, PAD, STRIDED, SV_SWEEP, TOL, _bits_differ, _both_forms, _ids, _len,
                               _pairs, _random_case, _report, _t)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, HKV = 2, 4, 2                                     # of _random_case
FAMILIES = BOUNDARY + MERGE + MANY_CHUNKS + [(128, 700, 2)]
UNDER_LEN = [(128, 700, 2, sv) for sv in SV_SWEEP]
NAN16, INF16 = 0x7E00, 0x7C00                           # fp16 bit patterns


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


@pytest.fixture(scope="module")
def oc():
    import eetq_amd.ops_ctypes as o
    return o


def _bits(x):
    return x.contiguous().view(torch.int16)


# ---- the quantising write: edge rows and wide heads ----------------------------------------------------------------------------
def _write_and_check(ops, q_np, k_np, v_np, table_np, pos_np, base, dev_base, identity):
    """q [B, T, H, D], k / v [B, T, Hkv, D] as slices of one fused projection row, written at rows base .. base + T - 1 of caches
    with fill patterns.  q and the rotated k equal the fp16 kernel's rotation bit for bit (and k is unchanged when the table is
    the identity), v is untouched, bytes and scale bits equal NumPy (rope_neox_f16, then quantize_rows), every other cache row
    keeps its pattern."""
    nb, T, nh, D = q_np.shape
    nkv = k_np.shape[2]
    S = base + T + 5
    qkv_np = np.concatenate([q_np.reshape(nb, T, -1), k_np.reshape(nb, T, -1), v_np.reshape(nb, T, -1)], axis=-1)

    def views(buf):
        return (buf[..., : nh * D].unflatten(-1, (nh, D)), buf[..., nh * D: (nh + nkv) * D].unflatten(-1, (nkv, D)),
                buf[..., (nh + nkv) * D:].unflatten(-1, (nkv, D)))

    qkv, qkv16 = _t(qkv_np), _t(qkv_np)
    q, k, v = views(qkv)
    table, pos = _t(table_np), _t(pos_np)
    k8 = torch.full((nb, nkv, S, D), 0x55, dtype=torch.int8, device=DEV)
    v8 = torch.full((nb, nkv, S, D), 0x33, dtype=torch.int8, device=DEV)
    sc = torch.full((nb, nkv, S, 2), 7.0, dtype=torch.float16, device=DEV)
    row = dict(first_row_dev=torch.tensor(base, dtype=torch.int64, device=DEV)) if dev_base else dict(first_row=base)
    ops.rotary_embedding_neox_kvcache_prefill_i8(pos, q, k, v, D, table, k8, v8, sc, **row)
    q16, k16, v16 = views(qkv16)
    kc16 = torch.zeros((nb, nkv, S, D), dtype=torch.float16, device=DEV)
    ops.rotary_embedding_neox_kvcache_prefill(pos, q16, k16, v16, D, table, kc16, torch.zeros_like(kc16), first_row=base)
    assert torch.equal(_bits(q), _bits(q16)), "q: the fp16 kernel's rotation"
    assert torch.equal(_bits(k.transpose(1, 2)), _bits(kc16[:, :, base: base + T])), "k in place: the fp16 kernel's rotation"
    assert torch.equal(_bits(v), _bits(_t(v_np))), "v is read only"
    if identity:
        assert torch.equal(_bits(k), _bits(_t(k_np))) and torch.equal(_bits(q), _bits(_t(q_np))), "the identity rotation"
    kr = ac.rope_neox_f16(k_np.reshape(nb * T, nkv, D), table_np, pos_np.reshape(-1)).reshape(nb, T, nkv, D).transpose(0, 2, 1, 3)
    assert np.array_equal(kr.view(np.int16), kc16[:, :, base: base + T].cpu().numpy().view(np.int16))
    ek8, eks = k8c.quantize_rows(kr)
    ev8, evs = k8c.quantize_rows(v_np.transpose(0, 2, 1, 3))
    got_k, got_v = k8[:, :, base: base + T].cpu().numpy(), v8[:, :, base: base + T].cpu().numpy()
    got_s = sc[:, :, base: base + T].cpu().numpy().view(np.uint16)
    exp_s = k8c.scale_pairs(eks, evs).view(np.uint16)
    bad_s = np.argwhere(got_s != exp_s)
    assert not len(bad_s), "scale bits differ at (b, kv head, token, k|v) %s: got %s, expected %s" % (
        bad_s[:6].tolist(), [hex(got_s[tuple(i)]) for i in bad_s[:6]], [hex(exp_s[tuple(i)]) for i in bad_s[:6]])
    for name, got, exp in (("K", got_k, ek8), ("V", got_v, ev8)):
        bad = np.argwhere((got != exp).any(-1))
        assert not len(bad), "%s bytes differ in %d rows, first (b, kv head, token) %s: got %s, expected %s" % (
            name, len(bad), bad[:6].tolist(), got[tuple(bad[0])][:12].tolist(), exp[tuple(bad[0])][:12].tolist())
    keep = torch.ones(S, dtype=torch.bool, device=DEV)
    keep[base: base + T] = False
    assert (k8[:, :, keep] == 0x55).all() and (v8[:, :, keep] == 0x33).all() and (sc[:, :, keep] == 7.0).all()


def _laid_out(rows, groups, lanes):
    """rows [R, D] -> K [groups, lanes, D] (zero rows behind the last one) and V: the same list rolled by one, so that a row's
    K and V scales differ"""
    R, D = rows.shape
    padded = np.zeros((groups * lanes, D), dtype=np.float16)
    padded[:R] = rows
    return padded.reshape(groups, lanes, D), np.roll(padded, 1, axis=0).reshape(groups, lanes, D)


@pytest.mark.parametrize("dev_base", [False, True], ids=["host-row", "device-row"])
@pytest.mark.parametrize("D", [64, 128])
def test_edge_rows_through_the_prompt_writer(ops, D, dev_base):
    """Every edge row once as K and once as V, laid over (token, KV head) with 4 KV heads; the second batch row holds them in
    reverse order.  The table is the identity, so K reaches the quantiser as built."""
    rows, _ = k8c.edge_rows_flat(D)
    nkv = 4
    T = -(-len(rows) // nkv)
    k0, v0 = _laid_out(rows, T, nkv)
    k_np = np.stack([k0, k0.reshape(-1, D)[::-1].reshape(T, nkv, D)])
    v_np = np.stack([v0, v0.reshape(-1, D)[::-1].reshape(T, nkv, D)])
    q_np = ac.normal_f16(np.random.default_rng(D), (2, T, nkv, D))
    pos_np = np.stack([np.arange(T, dtype=np.int64), (np.arange(T, dtype=np.int64) * 5) % T])
    _write_and_check(ops, q_np, k_np, v_np, k8c.identity_table(D, T), pos_np, 3, dev_base, identity=True)


WIDE = [(40, 128, 1, 2), (33, 128, 2, 3), (36, 64, 1, 2), (65, 64, 1, 1)]


def _per_head(rng, shape):
    """N(0, 1) scaled by 2^(head % 5) (exact in fp16): a scale paired with the wrong head shows.  shape [..., heads, D]"""
    x = ac.normal_f16(rng, shape)
    return (x * (2.0 ** (np.arange(shape[-2]) % 5)).astype(np.float16)[:, None]).astype(np.float16)


@pytest.mark.parametrize("dev_base", [False, True], ids=["host-row", "device-row"])
@pytest.mark.parametrize("nh,D,nb,T", WIDE, ids=_ids(WIDE))
def test_quantising_write_with_many_heads(ops, nh, D, nb, T, dev_base):
    """Heads x D / 16 (K) or D / 8 (V) threads beyond the 256 of a workgroup: 40 x 128 is the benchmarked shape (K a second trip
    of one wave, V three trips), 33 x 128 ends K in a single 8-lane group and V in a single 16-lane group, 36 x 64 ends V in
    half a wave, 65 x 64 ends K in a single 4-lane group."""
    rng = np.random.default_rng(1000 * nh + D)
    q_np, k_np, v_np = _per_head(rng, (nb, T, nh, D)), _per_head(rng, (nb, T, nh, D)), _per_head(rng, (nb, T, nh, D))
    base = 7
    pos_np = (base + np.arange(T, dtype=np.int64))[None, :].repeat(nb, 0) + np.array([[3], [14]])[:nb]
    _write_and_check(ops, q_np, k_np, v_np, ac.rope_table(D, 64), pos_np, base, dev_base, identity=False)


# ---- the one-launch form's quantiser ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
def test_edge_rows_through_the_one_launch_form(ops, D, splits):
    """Every edge row as the new token's K and (rolled by one) V, laid over (batch row, KV head) with H = Hkv = 4, behind a
    random quantised cache of 40 rows whose counter stands at 39: the written bytes and scale pair equal NumPy's, caches and
    outputs are bit-identical to the write launch followed by the two-launch attention, the tickets are zero again
    (_both_forms), and the output is finite."""
    rows, _ = k8c.edge_rows_flat(D)
    S, nh = 40, 4
    nb = -(-len(rows) // nh)
    k_np, v_np = _laid_out(rows, nb, nh)
    c = ac.random_case(nb, nh, nh, S, D, seed=40 + D)
    qc = k8c.quantize_cache(c["k"], c["v"])
    ek8, eks = k8c.quantize_rows(k_np)
    ev8, evs = k8c.quantize_rows(v_np)
    table = _t(k8c.identity_table(D, 64))
    pos = _t(np.random.default_rng(D + splits).integers(0, 64, size=nb).astype(np.int64))
    for slot in (0, S - 1):
        out, q_rot, cache = _both_forms(ops, D, S, splits, _t(c["q"]), _t(k_np), _t(v_np), pos, table, _t(qc["k8"]), _t(qc["v8"]),
                                        _t(qc["scales"]), slot, None, c["scale"])
        assert torch.isfinite(out).all()
        assert torch.equal(_bits(q_rot), _bits(_t(c["q"]))), "the identity rotation"
        # the rows as built, not through the NumPy rotation
        assert np.array_equal(cache[0][:, :, slot].cpu().numpy(), ek8) and np.array_equal(cache[1][:, :, slot].cpu().numpy(), ev8)
        assert np.array_equal(cache[2][:, :, slot].cpu().numpy().view(np.uint16), k8c.scale_pairs(eks, evs).view(np.uint16))


def test_one_launch_form_with_forty_heads(ops):
    """The benchmarked width, H = Hkv = 40 at D = 128, two chunks: the written row equals NumPy's and both forms agree."""
    nh, D, S, splits = 40, 128, 96, 2
    rng = np.random.default_rng(4096)
    c = ac.random_case(1, nh, nh, S, D, seed=41)
    qc = k8c.quantize_cache(c["k"], c["v"])
    k_new, v_new = _per_head(rng, (1, nh, D)), _per_head(rng, (1, nh, D))
    table, pos = _t(ac.rope_table(D, 256)), _t(np.array([97], dtype=np.int64))
    for slot in (0, S - 1):
        out, _, _ = _both_forms(ops, D, S, splits, _t(c["q"]), _t(k_new), _t(v_new), pos, table, _t(qc["k8"]), _t(qc["v8"]),
                                _t(qc["scales"]), slot, None, c["scale"])
        assert torch.isfinite(out).all()


# ---- the attention families the fp16 kernel has ----------------------------------------------------------------------------------
VAR_B, VAR_H, MASK_PAD = 16, 4, 40


@functools.lru_cache(maxsize=len(FAMILIES))
def _var_case(D, S):
    """attn_cases.hot_base at 16 x 4 heads, quantised; only what the launches need stays (on the device)"""
    c = ac.hot_base(VAR_B, VAR_H, S, D, seed=1000 * D + S)
    qc = k8c.quantize_cache(c["k"], c["v"])
    hot8, hots = k8c.quantize_rows(c["hot"])
    hotter8, hotters = k8c.quantize_rows(c["hotter"])
    hotd, hotterd = k8c.dequantize_rows(hot8, hots), k8c.dequantize_rows(hotter8, hotters)
    q64 = c["q"].astype(np.float64)
    gap = ac.hot_gap(c["q"], qc["kd"], hotd, c["scale"])
    gap_hotter = float((((q64 * hotterd).sum(-1) - (q64 * hotd).sum(-1)) * c["scale"]).min())
    print("kv8 edges D=%d S=%d: quantised hot key gap %.1f, hotter over hot %.1f" % (D, S, gap, gap_hotter))
    return dict(q=_t(c["q"]), k8=_t(qc["k8"]), v8=_t(qc["v8"]), sc=_t(qc["scales"]), hot8=_t(hot8), hots=_t(hots),
                hotter8=_t(hotter8), hotters=_t(hotters), exp=_t(k8c.hot_value(qc["v8"], qc["scales"][..., 1])),
                scale=c["scale"], gap=gap, gap_hotter=gap_hotter)


def _strided_views(k8, v8, sc, pad_scale=9.0):
    """the layouts of test_gpu_kv8_attn.test_hot_row_strided_cache: K a permuted view of [B, S, H, D] storage, V rows padded to
    D + 8 bytes, the scales a view of [B, H, S, 4] storage"""
    nb, nh, S, D = k8.shape
    k = torch.empty((nb, S, nh, D), dtype=torch.int8, device=DEV).permute(0, 2, 1, 3).copy_(k8)
    v = torch.full((nb, nh, S, D + 8), 5, dtype=torch.int8, device=DEV)[..., :D].copy_(v8)
    s = torch.full((nb, nh, S, 4), pad_scale, dtype=torch.float16, device=DEV)[..., :2].copy_(sc)
    assert not k.is_contiguous() and not v.is_contiguous() and not s.is_contiguous() and k.stride() != v.stride()
    return k, v, s


@pytest.mark.parametrize("layout", ["contiguous", "strided"])
@pytest.mark.parametrize("D,S,splits", FAMILIES, ids=_ids(FAMILIES))
def test_hot_row_past_the_valid_length(ops, D, S, splits, layout):
    """Every row >= Sv carries the hotter key's bytes under its full scale (and a 0x7F V row); then, in a second pass, NaN and
    +Inf scale bit patterns over 0x7F bytes.  Rows that do not count return bytes 0 and scale 0, so the answer is the hot row
    among the valid ones bit for bit, and 0 * NaN never happens.  Sv ragged and Sv a whole number of blocks."""
    c = _var_case(D, S)
    assert c["gap"] >= ac.GAP_MIN and c["gap_hotter"] >= ac.GAP_MIN
    ib, ih = _pairs(VAR_B, VAR_H)
    for sv in (S - blk(D) - 5, (nblocks(D, S) // 2) * blk(D)):
        r = _t(_edge_rows(D, S, splits, sv, VAR_B * VAR_H, seed=sv))
        for poison in (False, True):
            k8, v8, sc = c["k8"].clone(), c["v8"].clone(), c["sc"].clone()
            k8[ib, ih, r] = c["hot8"].reshape(VAR_B * VAR_H, D)
            sc[ib, ih, r, 0] = c["hots"].reshape(VAR_B * VAR_H)
            v8[:, :, sv:] = 0x7F
            if poison:
                k8[:, :, sv:] = 0x7F
                pat = torch.tensor([[NAN16, INF16], [INF16, NAN16]], dtype=torch.int16, device=DEV).repeat(-(-(S - sv) // 2), 1)
                sc.view(torch.int16)[:, :, sv:] = pat[: S - sv]
                assert not torch.isfinite(sc[:, :, sv:]).any() and torch.isnan(sc[:, :, sv:]).any()
            else:
                k8[:, :, sv:] = c["hotter8"][:, :, None]
                sc[:, :, sv:, 0] = c["hotters"][:, :, None]
            if layout == "strided":
                k8, v8, sc = _strided_views(k8, v8, sc, float("nan") if poison else 9.0)
            out = ops.decode_attention_i8kv(c["q"], k8, v8, sc, scaling=c["scale"], splits=splits, kv_len=_len(sv))
            assert not torch.isnan(out).any(), (sv, poison)
            _report(D, [(r, _bits_differ(out, c["exp"][ib, ih, r]))])


@pytest.mark.parametrize("D,S,splits", FAMILIES, ids=_ids(FAMILIES))
def test_hot_row_by_mask_alone(ops, D, S, splits):
    """K bytes 0: the scores are the mask.  mask[b, r_b] = 0, every other element -200 (finite in fp16), rows S + 40 long: pins
    the mask element to its position and the batch stride, in the MASK instantiation with its three descriptors."""
    c = _var_case(D, S)
    assert 200.0 >= ac.GAP_MIN                     # the scores are 0 everywhere: the gap is the mask's own
    k8 = torch.zeros_like(c["k8"])
    rows = _edge_rows(D, S, splits, S, 2 * VAR_B, seed=S + splits)
    ar = torch.arange(VAR_B, device=DEV)
    fails = []
    for r in (_t(rows[:VAR_B]), _t(rows[VAR_B:])):
        mask = torch.full((VAR_B, S + MASK_PAD), -200.0, dtype=torch.float16, device=DEV)
        mask[:, S:] = 0.0   # never read: beyond the cache
        mask[ar, r] = 0.0
        out = ops.decode_attention_i8kv(c["q"], k8, c["v8"], c["sc"], mask=mask, scaling=c["scale"], splits=splits)
        fails.append((r.repeat_interleave(VAR_H), _bits_differ(out, c["exp"][ar, :, r])))
    _report(D, fails)


@pytest.mark.parametrize("D,S,splits", FAMILIES, ids=_ids(FAMILIES))
def test_masked_hot_row(ops, D, S, splits):
    """A hotter key at r1 under mask -inf: the answer is the second hot row -- one row after r1, one block after, half a cache
    away, one row before (head by head)."""
    c = _var_case(D, S)
    assert c["gap"] >= ac.GAP_MIN and c["gap_hotter"] >= ac.GAP_MIN
    ib, ih = _pairs(VAR_B, VAR_H)
    ar = torch.arange(VAR_B, device=DEV)
    r1 = _t(_edge_rows(D, S, splits, S, VAR_B, seed=7 * S + splits))
    off = torch.tensor([1, blk(D), S // 2 + 3, S - 1], device=DEV)
    r2 = (r1[:, None] + off[None, :]).flatten() % S
    k8, sc = c["k8"].clone(), c["sc"].clone()
    k8[ar, :, r1] = c["hotter8"]
    sc[ar, :, r1, 0] = c["hotters"]
    k8[ib, ih, r2] = c["hot8"].reshape(VAR_B * VAR_H, D)
    sc[ib, ih, r2, 0] = c["hots"].reshape(VAR_B * VAR_H)
    mask = torch.zeros((VAR_B, S + MASK_PAD), dtype=torch.float16, device=DEV)
    mask[ar, r1] = float("-inf")
    out = ops.decode_attention_i8kv(c["q"], k8, c["v8"], sc, mask=mask, scaling=c["scale"], splits=splits)
    _report(D, [(r2, _bits_differ(out, c["exp"][ib, ih, r2]))])


@pytest.mark.parametrize("D,S,splits", FAMILIES, ids=_ids(FAMILIES))
def test_hot_v_rows_from_the_edge_rows(ops, D, S, splits):
    """The hot row's V is an edge row: the tiny rows (V scales 0, 0, u, u, u, 2u, 2u, 8u with u = 2^-24), the zero row, the
    amax-65504 row (scale 516), the tie rows and the first sweep rows.  out == fp16(vs * v8), subnormal where that is; by value
    where the scale is 0 (see the file's docstring)."""
    c = _var_case(D, S)
    assert c["gap"] >= ac.GAP_MIN
    n = VAR_B * VAR_H
    fam = k8c.edge_rows(D)
    picked = np.concatenate([fam["tiny"], fam["zero"], fam["extreme"], fam["ties"], fam["sweep"]])[:n]
    e8, es = k8c.quantize_rows(picked)
    assert len(picked) == n and (es == 0).sum() == 3 and (es.view(np.uint16) == 1).sum() == 3 and (es == 516).sum() == 1
    with np.errstate(over="ignore"):               # 516 * 127 = 65532 is inf in fp16, for NumPy and for the kernel
        exp = _t(k8c.hot_value(e8, es))
    assert torch.isinf(exp).sum() == 2
    ib, ih = _pairs(VAR_B, VAR_H)
    r = _t(_edge_rows(D, S, splits, S, n, seed=3 * S + splits))
    k8, v8, sc = c["k8"].clone(), c["v8"].clone(), c["sc"].clone()
    k8[ib, ih, r] = c["hot8"].reshape(n, D)
    sc[ib, ih, r, 0] = c["hots"].reshape(n)
    v8[ib, ih, r] = _t(e8)
    sc[ib, ih, r, 1] = _t(es)
    out = ops.decode_attention_i8kv(c["q"], k8, v8, sc, scaling=c["scale"], splits=splits)
    assert not torch.isnan(out).any()
    by_value = (out.reshape(n, D) != exp).any(-1)
    bad = torch.where(_t(es == 0), by_value, _bits_differ(out, exp))
    _report(D, [(r, bad)])


@pytest.mark.parametrize("D,S,splits,sv", UNDER_LEN, ids=_ids(UNDER_LEN))
def test_random_masks_under_kv_len(ops, D, S, splits, sv):
    """Grouped-query heads, an aperiodic finite / -inf mask and a valid length from the device, in the MASK instantiation."""
    c, qc = _random_case(D, S)
    mask = ac.random_mask(B, S + PAD, seed=S + D + splits + sv)
    out = ops.decode_attention_i8kv(_t(c["q"]), _t(qc["k8"]), _t(qc["v8"]), _t(qc["scales"]), mask=_t(mask), scaling=c["scale"],
                                    splits=splits, kv_len=_len(sv))
    ref = ac.reference(c["q"], qc["kd"], qc["vd"], sv, c["scale"], mask)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max()
    print("kv8 edges random D=%d S=%d splits=%d Sv=%d: max |out - ref| %.3e" % (D, S, splits, sv, err))
    assert torch.isfinite(out).all() and err < TOL
    if sv == 0:
        assert torch.count_nonzero(out) == 0


FULLY_MASKED = [(128, 700, 2), (64, 96, 33)]


@pytest.mark.parametrize("D,S,splits", FULLY_MASKED, ids=_ids(FULLY_MASKED))
def test_fully_masked_batch_row(ops, D, S, splits):
    """The mask of batch row 0 is -inf everywhere (the new token's row included): zeros there, the reference elsewhere, in the
    two-launch form and in the one-launch form."""
    c, qc = _random_case(D, S)
    mask = ac.random_mask(B, S + PAD, seed=S + D)
    mask[0] = -np.inf
    q, k8, v8, sc = _t(c["q"]), _t(qc["k8"]), _t(qc["v8"]), _t(qc["scales"])
    out = ops.decode_attention_i8kv(q, k8, v8, sc, mask=_t(mask), scaling=c["scale"], splits=splits)
    ref = ac.reference(c["q"], qc["kd"], qc["vd"], S, c["scale"], mask)
    assert not ref[0].any() and np.abs(ref[1]).max() > 0.01
    assert torch.isfinite(out).all() and torch.count_nonzero(out[0]) == 0
    assert np.abs(out.cpu().numpy().astype(np.float64) - ref).max() < TOL
    rng = np.random.default_rng(S)
    k_new, v_new = _t(ac.normal_f16(rng, (B, HKV, D))), _t(ac.normal_f16(rng, (B, HKV, D)))
    table, pos = _t(ac.rope_table(D, 2048)), _t(np.array([700, 31], dtype=np.int64))
    for slot in (0, S - 1):
        out, q_rot, cache = _both_forms(ops, D, S, splits, q, k_new, v_new, pos, table, k8, v8, sc, slot, _t(mask), c["scale"])
        s_np = cache[2].cpu().numpy()
        ref = ac.reference(q_rot.cpu().numpy(), k8c.dequantize_rows(cache[0].cpu().numpy(), s_np[..., 0]),
                           k8c.dequantize_rows(cache[1].cpu().numpy(), s_np[..., 1]), S, c["scale"], mask)
        assert torch.isfinite(out).all() and torch.count_nonzero(out[0]) == 0, slot
        assert np.abs(out.cpu().numpy().astype(np.float64) - ref).max() < TOL, slot


# ---- both bindings -------------------------------------------------------------------------------------------------------------
def _strided_random(D, S):
    """the caches of test_gpu_kv8_attn.test_random_strided_cache, with the storage they are views of"""
    c, qc = _random_case(D, S)
    bk = torch.full((B, HKV, S, D + 8), 5, dtype=torch.int8, device=DEV)
    bv = torch.empty((B, S, HKV, D), dtype=torch.int8, device=DEV)
    bs = torch.full((B, HKV, S, 6), 9.0, dtype=torch.float16, device=DEV)
    k8, v8, sc = bk[..., :D], bv.permute(0, 2, 1, 3), bs[..., 2:4]
    k8.copy_(_t(qc["k8"])), v8.copy_(_t(qc["v8"])), sc.copy_(_t(qc["scales"]))
    return c, qc, (k8, v8, sc), (bk, bv, bs)


def _same_storage(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))


@pytest.mark.parametrize("D,S,splits", STRIDED, ids=_ids(STRIDED))
def test_both_bindings_decode_attention(ops, oc, D, S, splits):
    """eetq_amd.ops_ctypes against the compiled module on strided caches (byte strides for the caches, fp16-element strides
    for the scales), with a mask, a device length, a bias and an advanced counter: the same output bits, the same counter."""
    mask = _t(ac.random_mask(B, S + PAD, seed=S + D))
    res = []
    for mod in (ops, oc):
        c, qc, views, base = _strided_random(D, S)
        cnt = torch.tensor(S - 201, dtype=torch.int64, device=DEV)
        out = mod.decode_attention_i8kv(_t(c["q"]), *views, mask=mask, scaling=c["scale"], splits=splits, kv_len=cnt, kv_len_bias=1,
                                        advance=cnt)
        res.append((out, int(cnt.item()), base))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and res[0][1] == res[1][1] == S - 200
    assert _same_storage(res[0][2], res[1][2])
    ref = ac.reference(c["q"], qc["kd"], qc["vd"], S - 200, c["scale"], mask.cpu().numpy())
    assert np.abs(res[1][0].cpu().numpy().astype(np.float64) - ref).max() < TOL


@pytest.mark.parametrize("D,S,splits", STRIDED, ids=_ids(STRIDED))
def test_both_bindings_one_launch_form(ops, oc, D, S, splits):
    """The same for the one-launch form: output bits, the written caches and scales down to the bytes between the rows, the
    counter and the tickets."""
    mask = _t(ac.random_mask(B, S + PAD, seed=S + D + 1))
    rng = np.random.default_rng(S + 9)
    k_new, v_new = _t(ac.normal_f16(rng, (B, HKV, D))), _t(ac.normal_f16(rng, (B, HKV, D)))
    table, pos = _t(ac.rope_table(D, 2048)), _t(np.array([11, 1900], dtype=np.int64))
    slot = S - 200
    res = []
    for mod in (ops, oc):
        c, qc, views, base = _strided_random(D, S)
        cnt = torch.tensor(slot, dtype=torch.int64, device=DEV)
        tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)
        out = mod.rope_decode_attention_i8kv(pos, _t(c["q"]), k_new, v_new, table, *views, tickets,
                                             slots=torch.full((B,), slot, dtype=torch.int64, device=DEV), mask=mask,
                                             scaling=c["scale"], splits=splits, kv_len=cnt, kv_len_bias=1, advance=cnt)
        assert torch.count_nonzero(tickets) == 0
        res.append((out, int(cnt.item()), base, views))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and res[0][1] == res[1][1] == slot + 1
    assert _same_storage(res[0][2], res[1][2])
    # the row is NumPy's, and only the row was written (the bytes between the rows keep their fill)
    kr = ac.rope_neox_f16(k_new.cpu().numpy(), table.cpu().numpy(), pos.cpu().numpy())
    ek8, eks = k8c.quantize_rows(kr)
    ev8, evs = k8c.quantize_rows(v_new.cpu().numpy())
    (bk, bv, bs), (k8, v8, sc) = res[1][2], res[1][3]
    assert np.array_equal(k8[:, :, slot].cpu().numpy(), ek8) and np.array_equal(v8[:, :, slot].cpu().numpy(), ev8)
    assert np.array_equal(sc[:, :, slot].cpu().numpy().view(np.uint16), k8c.scale_pairs(eks, evs).view(np.uint16))
    assert (bk[..., D:] == 5).all() and (bs[..., :2] == 9.0).all() and (bs[..., 4:] == 9.0).all()
    keep = torch.arange(S, device=DEV) != slot
    assert torch.equal(k8[:, :, keep], _t(qc["k8"])[:, :, keep]) and torch.equal(v8[:, :, keep], _t(qc["v8"])[:, :, keep])
    assert torch.equal(_bits(sc[:, :, keep]), _bits(_t(qc["scales"])[:, :, keep]))


@pytest.mark.parametrize("D", [64, 128])
def test_both_bindings_quantising_write(ops, oc, D):
    """The write entry on caches whose rows are D + 8 bytes apart and scales that are a view: the same q, k, bytes and scales."""
    T, S, base = 3, 20, 6
    rng = np.random.default_rng(D + 2)
    qkv_np = ac.normal_f16(rng, (B, T, (H + 2 * HKV) * D))
    table, pos = _t(ac.rope_table(D, 64)), _t(np.array([[6, 7, 8], [20, 21, 22]], dtype=np.int64))
    res = []
    for mod in (ops, oc):
        qkv = _t(qkv_np)
        q, k, v = (qkv[..., : H * D].unflatten(-1, (H, D)), qkv[..., H * D: (H + HKV) * D].unflatten(-1, (HKV, D)),
                   qkv[..., (H + HKV) * D:].unflatten(-1, (HKV, D)))
        bk = torch.full((B, HKV, S, D + 8), 0x55, dtype=torch.int8, device=DEV)
        bv = torch.full((B, HKV, S, D + 8), 0x33, dtype=torch.int8, device=DEV)
        bs = torch.full((B, HKV, S, 6), 7.0, dtype=torch.float16, device=DEV)
        mod.rotary_embedding_neox_kvcache_prefill_i8(pos, q, k, v, D, table, bk[..., :D], bv[..., :D], bs[..., 2:4],
                                                     first_row_dev=torch.tensor(base, dtype=torch.int64, device=DEV))
        res.append((qkv, bk, bv, bs))
    for a, b in zip(res[0], res[1]):      # the whole projection buffer and the three storages
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b)
    qkv, bk, bv, bs = res[1]
    k_np = qkv_np[..., H * D: (H + HKV) * D].reshape(B * T, HKV, D)
    kr = ac.rope_neox_f16(k_np, table.cpu().numpy(), pos.cpu().numpy().reshape(-1)).reshape(B, T, HKV, D).transpose(0, 2, 1, 3)
    ek8, eks = k8c.quantize_rows(kr)
    ev8, evs = k8c.quantize_rows(qkv_np[..., (H + HKV) * D:].reshape(B, T, HKV, D).transpose(0, 2, 1, 3))
    assert np.array_equal(bk[:, :, base: base + T, :D].cpu().numpy(), ek8) and np.array_equal(bv[:, :, base: base + T, :D].cpu().numpy(), ev8)
    assert np.array_equal(bs[:, :, base: base + T, 2:4].cpu().numpy().view(np.uint16), k8c.scale_pairs(eks, evs).view(np.uint16))
    keep = torch.ones(S, dtype=torch.bool, device=DEV)
    keep[base: base + T] = False
    assert (bk[:, :, keep] == 0x55).all() and (bv[:, :, keep] == 0x33).all() and (bs[:, :, keep] == 7.0).all()
    assert (bk[..., D:] == 0x55).all() and (bv[..., D:] == 0x33).all() and (bs[..., :2] == 7.0).all() and (bs[..., 4:] == 7.0).all()


def _entry_call(mod, entry, q, k8, v8, sc, nkv=HKV):
    nb, _, D = q.shape
    S = k8.shape[2]
    k_new = torch.zeros((nb, nkv, D), dtype=torch.float16, device=DEV)
    table = _t(ac.rope_table(D, 64))
    pos = torch.zeros(nb, dtype=torch.int64, device=DEV)
    if entry == "decode":
        return mod.decode_attention_i8kv(q, k8, v8, sc, splits=1)
    if entry == "one-launch":
        return mod.rope_decode_attention_i8kv(pos, q, k_new, k_new.clone(), table, k8, v8, sc,
                                              torch.zeros(nb * q.shape[1] + 1, dtype=torch.int32, device=DEV),
                                              slots=torch.full((nb,), S - 1, dtype=torch.int64, device=DEV), splits=1)
    return mod.rotary_embedding_neox_kvcache_prefill_i8(pos[:, None], q[:, None], k_new[:, None], k_new.clone()[:, None], D, table,
                                                        k8, v8, sc, first_row=0)


@pytest.mark.parametrize("entry", ["decode", "one-launch", "write"])
def test_both_bindings_refuse_alike(ops, oc, entry):
    """A cache stride that is no multiple of 8 bytes, an odd scale stride, a float32 query, mismatched KV heads: the same
    exception type from both bindings, before any launch; the arguments they are derived from pass."""
    D, S = 64, 32
    q = torch.zeros((B, H, D), dtype=torch.float16, device=DEV)

    def caches(nkv=HKV, row=D, pair=2):
        return (torch.zeros((B, nkv, S, row), dtype=torch.int8, device=DEV)[..., :D],
                torch.zeros((B, nkv, S, row), dtype=torch.int8, device=DEV)[..., :D],
                torch.zeros((B, nkv, S, pair), dtype=torch.float16, device=DEV)[..., :2])

    bad = {"cache stride": (q, caches(row=D + 4)), "scale stride": (q, caches(pair=3)), "float32 query": (q.float(), caches()),
           "kv heads": (q, caches(nkv=3))}
    for mod in (ops, oc):
        _entry_call(mod, entry, q, *caches())
    torch.cuda.synchronize()
    for what, (qq, cc) in bad.items():
        raised = []
        for mod in (ops, oc):
            with pytest.raises(Exception) as info:
                _entry_call(mod, entry, qq, *cc)
            raised.append(info.type)
        assert raised[0] is raised[1] is RuntimeError, (what, raised)
