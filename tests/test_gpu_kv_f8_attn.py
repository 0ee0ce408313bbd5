"""The fp8 (e4m3) KV cache's kernels (KvF8 in eetq_amd/csrc/attn_decode.hip, the quantising write of norm_rope.hip; DESIGN.md
4.7e) with the input families of tests/attn_cases.py.  The quantiser is torch on the CPU:
``(x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn)``; references are float64 on the dequantised rows.

TOL is that of test_gpu_kv8_attn.py.  B = 2, H = 4, Hkv = 2; the hot-row family gives every head its own rows (Hkv = H)."""
import functools
import itertools

import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-3
B, H, HKV = 2, 4, 2
PAD = 24
SHAPES = [(128, 700, 2), (64, 512, 1), (64, 513, 1), (128, 1040, 17), (64, 1040, 65)]
UNDER_LEN = [(128, 700, 2, sv) for sv in (0, 1, 16, 17, 257, 700)]
SCALES = [(1.0, 1.0), (0.37, 2.5)]
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def quant(x, s):
    """the format's rule, on the CPU; x fp16 (NumPy or torch), s float32 broadcastable -> float8_e4m3fn"""
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.cpu()
    return (x.float() / s).clamp(-448, 448).to(F8)


def per_head(scales, col):   # column `col` of scales [Hkv, 2] shaped for rows [B, Hkv, S, D]
    return scales[:, col].reshape(1, -1, 1, 1)


def dequant(x8, s):
    return (x8.cpu().float() * s).double().numpy()


def _bytes(x8):
    return x8.cpu().view(torch.uint8)


def _bits_differ(out, exp):
    D = out.shape[-1]
    return (out.reshape(-1, D).view(torch.int16) != exp.reshape(-1, D).view(torch.int16)).any(-1)


# ---- the quantising cache write ------------------------------------------------------------------------------------------
def _write_case(ops, D, s, dev_base):
    bits = np.arange(1 << 16, dtype=np.uint16)
    vals = bits[(bits & 0x7C00) != 0x7C00].view(np.float16)
    assert vals.size == 63488
    T, base = vals.size // (B * HKV * D), 3
    S = base + T
    rng = np.random.default_rng(D)
    qkv = torch.empty((B, T, (H + 2 * HKV) * D), dtype=torch.float16, device=DEV)
    q, k, v = (qkv[..., : H * D].unflatten(-1, (H, D)), qkv[..., H * D: (H + HKV) * D].unflatten(-1, (HKV, D)),
               qkv[..., (H + HKV) * D:].unflatten(-1, (HKV, D)))
    q.copy_(_t(ac.normal_f16(rng, (B, T, H, D))))
    k.copy_(_t(ac.normal_f16(rng, (B, T, HKV, D)) * np.float16(40)))      # beyond 448 * 0.37 now and then: the clamp
    v.copy_(_t(vals.reshape(B, T, HKV, D)))
    q16, k16 = q.clone(), k.clone()
    table = _t(ac.rope_table(D, 2048))
    pos = _t(np.arange(T, dtype=np.int64)[None, :].repeat(B, 0) + np.array([[0], [11]]))
    scales = torch.tensor([[s, s], [0.5, s]], dtype=torch.float32)
    k8 = torch.full((B, HKV, S, D), 0x55, dtype=torch.uint8, device=DEV).view(F8)
    v8 = torch.full((B, HKV, S, D), 0x33, dtype=torch.uint8, device=DEV).view(F8)
    ops.decode_dropped_steps(reset=True)
    row = dict(first_row_dev=torch.tensor(base + 1, dtype=torch.int64, device=DEV)) if dev_base else dict(first_row=base)
    ops.rotary_embedding_neox_kvcache_prefill_f8(pos, q, k, v, D, table, k8, v8, scales.to(DEV), **row)
    assert ops.decode_dropped_steps(reset=True) == (B if dev_base else 0)
    # the fp16 entry on a copy: the same q and k in place
    kc16 = torch.zeros((B, HKV, S, D), dtype=torch.float16, device=DEV)
    ops.rotary_embedding_neox_kvcache_prefill(pos, q16, k16, v.clone(), D, table, kc16, torch.zeros_like(kc16), first_row=base)
    n, b0 = (T - 1, base + 1) if dev_base else (T, base)            # (a dropped token is not rotated either)
    assert torch.equal(q[:, :n].contiguous().view(torch.int16), q16[:, :n].contiguous().view(torch.int16))
    assert torch.equal(k[:, :n].transpose(1, 2).contiguous().view(torch.int16), kc16[:, :, base: base + n].contiguous().view(torch.int16))
    ek8 = quant(kc16[:, :, base: base + n], per_head(scales, 0))
    ev8 = quant(v.transpose(1, 2)[:, :, :n], per_head(scales, 1))
    bad = _bytes(v8[:, :, b0:]) != _bytes(ev8)
    assert not bad.any(), "%d V bytes differ; first inputs %s" % (
        int(bad.sum()), v.transpose(1, 2)[:, :, :n].cpu()[bad][:8].tolist())
    assert torch.equal(_bytes(k8[:, :, b0:]), _bytes(ek8))
    assert (_bytes(k8[:, :, :b0]) == 0x55).all() and (_bytes(v8[:, :, :b0]) == 0x33).all(), "rows outside the range are untouched"


# ---- hot row -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _hot_case(D, S, ks, vs):
    c = ac.hot_base(B, H, S, D, seed=1000 * D + S)      # every head its own rows: k, v [B, H, S, D]
    ks32, vs32 = torch.tensor(ks, dtype=torch.float32), torch.tensor(vs, dtype=torch.float32)
    # hot_base keeps zeros out of V so that bit equality is value equality (an fp32 sum cannot return -0); values below half the
    # least e4m3 subnormal would bring them back as +-0 bytes, so they become 1.0, as nonzero_normal_f16 does with a zero
    v = c["v"].copy()
    v[(quant(v, vs32).float() == 0).numpy()] = np.float16(1.0)
    k8, v8, hot8 = quant(c["k"], ks32), quant(v, vs32), quant(c["hot"], ks32)
    assert (v8.float() != 0).all()
    gap = ac.hot_gap(c["q"], dequant(k8, ks32), dequant(hot8, ks32), c["scale"])
    print("kv f8 hot case D=%d S=%d scales (%g, %g): quantised hot key gap %.1f" % (D, S, ks, vs, gap))
    return dict(q=_t(c["q"]), k8=k8.to(DEV), v8=v8.to(DEV), hot8=hot8.to(DEV), exp=(v8.float() * vs32).half().to(DEV),
                scales=torch.tensor([[ks, vs]] * H, dtype=torch.float32, device=DEV), scale=c["scale"], gap=gap)


def _hot_row_case(ops, D, S, splits, ks, vs):
    c = _hot_case(D, S, ks, vs)
    assert c["gap"] >= ac.GAP_MIN
    ku = c["k8"].view(torch.uint8)
    ib, ih = torch.arange(B, device=DEV).repeat_interleave(H), torch.arange(H, device=DEV).repeat(B)
    rows, bad = [], []
    for launch in range(ac.sweep_launches(S, B * H)):
        r = _t(ac.sweep(S, B * H, launch))
        saved = ku[ib, ih, r].clone()
        ku[ib, ih, r] = c["hot8"].view(torch.uint8).reshape(B * H, D)
        out = ops.decode_attention_f8kv(c["q"], c["k8"], c["v8"], c["scales"], scaling=c["scale"], splits=splits)
        ku[ib, ih, r] = saved
        rows.append(r)
        bad.append(_bits_differ(out, c["exp"][ib, ih, r]))
    rows, bad = torch.cat(rows).cpu().numpy(), torch.cat(bad).cpu().numpy()
    assert not bad.any(), "%d of %d hot rows are not returned bit for bit; first rows: %s" % (bad.sum(), bad.size, rows[bad][:8].tolist())


# ---- random, both launch forms ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _random_case(D, S):
    c = ac.random_case(B, H, HKV, S, D, seed=3 * S + D)
    scales = torch.tensor([[0.37, 2.5], [0.74, 1.25]])   # the second kv head with scales of its own
    rng = np.random.default_rng(S + D)
    new = dict(k=ac.normal_f16(rng, (B, HKV, D)), v=ac.normal_f16(rng, (B, HKV, D)), table=ac.rope_table(D, 2048),
               pos=rng.integers(1, 2048, size=B).astype(np.int64))
    return c, scales, quant(c["k"], per_head(scales, 0)), quant(c["v"], per_head(scales, 1)), new


def _reference(q, k8, v8, scales, sv, scale, mask):
    return ac.reference(q, dequant(k8, per_head(scales, 0)), dequant(v8, per_head(scales, 1)), sv, scale, mask)


def _one_launch(ops, c, scales, k8, v8, new, slot, counter, mask, splits):
    """the step on copies of the caches -> (out, k8, v8, the counter, the tickets)"""
    k8, v8 = k8.to(DEV).clone(), v8.to(DEV).clone()
    nb, nh = c["q"].shape[:2]
    cnt = torch.tensor(counter, dtype=torch.int64, device=DEV)
    tickets = torch.zeros(nb * nh + 1, dtype=torch.int32, device=DEV)
    out = ops.rope_decode_attention_f8kv(_t(new["pos"]), _t(c["q"]), _t(new["k"]), _t(new["v"]), _t(new["table"]), k8, v8,
                                         scales.to(DEV), tickets, slots=torch.full((nb,), slot, dtype=torch.int64, device=DEV),
                                         mask=mask, scaling=c["scale"], splits=splits, kv_len=cnt, kv_len_bias=1, advance=cnt)
    return out, k8, v8, cnt, tickets


RANDOM = [s + (None,) for s in SHAPES] + UNDER_LEN


def _random_case_both_forms(ops, D, S, splits, sv):
    c, scales, k8, v8, new = _random_case(D, S)
    n = S if sv is None else sv
    q_rot = ac.rope_neox_f16(c["q"], new["table"], new["pos"])
    for m in (None, ac.random_mask(B, S + PAD, seed=S + D + splits)):
        mask = None if m is None else _t(m)
        out = ops.decode_attention_f8kv(_t(c["q"]), k8.to(DEV), v8.to(DEV), scales.to(DEV), mask=mask, scaling=c["scale"],
                                        splits=splits, kv_len=None if sv is None else torch.tensor(sv, device=DEV))
        err2 = np.abs(out.cpu().numpy().astype(np.float64) - _reference(c["q"], k8, v8, scales, n, c["scale"], m)).max()
        out1, k1, v1, _, _ = _one_launch(ops, c, scales, k8, v8, new, n - 1, n - 1, mask, splits)
        ref1 = _reference(q_rot if n else c["q"], k1, v1, scales, n, c["scale"], m)
        err1 = np.abs(out1.cpu().numpy().astype(np.float64) - ref1).max()
        print("kv f8 random D=%d S=%d splits=%d Sv=%d mask=%s: max |out - ref| two launches %.3e, one launch %.3e" % (
            D, S, splits, n, m is not None, err2, err1))
        assert torch.isfinite(out).all() and torch.isfinite(out1).all() and err2 < TOL and err1 < TOL
        if n == 0:
            assert torch.count_nonzero(out) == 0 and torch.count_nonzero(out1) == 0


# ---- one launch against two ----------------------------------------------------------------------------------------------
def _one_launch_equals_write_then_two_launches(ops, D, S, splits):
    c, scales, k8, v8, new = _random_case(D, S)
    blk = 4 * (64 // (D // 8))
    edges = [0, blk - 1, blk, 16 * splits * blk, S - 1]
    for slot in [r for r in dict.fromkeys(edges) if r < S]:
        for m in (None, ac.random_mask(B, S + PAD, seed=S + 2 * splits)):
            mask = None if m is None else _t(m)
            ka, va = k8.to(DEV).clone(), v8.to(DEV).clone()
            q_a, k_a = _t(c["q"]), _t(new["k"])
            cnt_a = torch.tensor(S - 1, dtype=torch.int64, device=DEV)
            ops.rotary_embedding_neox_kvcache_prefill_f8(_t(new["pos"])[:, None].contiguous(), q_a[:, None], k_a[:, None],
                                                         _t(new["v"])[:, None], D, _t(new["table"]), ka, va, scales.to(DEV),
                                                         first_row_dev=torch.tensor(slot, dtype=torch.int64, device=DEV))
            out_a = ops.decode_attention_f8kv(q_a, ka, va, scales.to(DEV), mask=mask, scaling=c["scale"], splits=splits,
                                              kv_len=cnt_a, kv_len_bias=1, advance=cnt_a)
            out_b, kb, vb, cnt_b, tickets = _one_launch(ops, c, scales, k8, v8, new, slot, S - 1, mask, splits)
            where = (slot, m is not None)
            assert torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)), where
            assert torch.equal(_bytes(ka), _bytes(kb)) and torch.equal(_bytes(va), _bytes(vb)), where
            assert torch.count_nonzero(tickets) == 0 and int(cnt_a.item()) == int(cnt_b.item()) == S, where
            kr = ac.rope_neox_f16(new["k"], new["table"], new["pos"])
            assert torch.equal(_bytes(kb[:, :, slot]), _bytes(quant(kr, scales[:, 0].reshape(1, -1, 1)))), where
            assert torch.equal(_bytes(vb[:, :, slot]), _bytes(quant(new["v"], scales[:, 1].reshape(1, -1, 1)))), where
            keep = torch.arange(S) != slot
            assert torch.equal(_bytes(kb)[:, :, keep], _bytes(k8)[:, :, keep]) and torch.equal(_bytes(vb)[:, :, keep], _bytes(v8)[:, :, keep])


def _slot_outside_the_cache(ops, slot):
    D, S, splits = 128, 700, 2
    c, scales, k8, v8, new = _random_case(D, S)
    ops.decode_dropped_steps(reset=True)
    out, k1, v1, _, _ = _one_launch(ops, c, scales, k8, v8, new, slot, 300, None, splits)
    assert ops.decode_dropped_steps(reset=True) == B
    exp = ops.decode_attention_f8kv(_t(c["q"]), k8.to(DEV), v8.to(DEV), scales.to(DEV), scaling=c["scale"], splits=splits,
                                    kv_len=torch.tensor(300, device=DEV), kv_len_bias=1)
    assert torch.equal(out.view(torch.int16), exp.view(torch.int16))
    assert torch.equal(_bytes(k1), _bytes(k8)) and torch.equal(_bytes(v1), _bytes(v8))


# ---- the tests: every case of a family in one test, the case printed before it runs --------------------------------------------
def _each(check, ops, cases):
    for case in cases:
        print(check.__name__, case)
        check(ops, *case)


def test_quantising_write_every_fp16_value(ops):
    """Every finite fp16 value goes in as V (63 488 / D rows over B x T x Hkv) at D = 64 / 128 and s = 1 / 0.37; K is random.  With
    the device base one row later the last token of each batch row falls outside the cache: dropped and counted, everything else as
    before."""
    _each(_write_case, ops, itertools.product((64, 128), (1.0, 0.37), (False, True)))


def test_hot_row_every_position(ops):
    """The quantised hot key at every position in turn (the cache is edited in place and restored), every shape at both scale
    pairs: out == fp16(fp32(v8[r]) * vs) bit for bit."""
    _each(_hot_row_case, ops, (shape + scales for shape in SHAPES for scales in SCALES))


def test_both_launch_forms(ops):
    """Random rows.  Two launches over the first sv rows and one launch whose new token is row sv - 1 (sv = 0: the slot is -1,
    nothing is written and nothing attended), each against float64 on the dequantised rows it attends, with and without a finite
    mask.  Then one launch against write + two launches with the new token's row at the block edges of a full cache (the counter at
    S - 1): outputs and caches bit-identical, the written row the quantiser's, only that row written, zero tickets, an advanced
    counter.  Then a slot outside the cache: neither written nor attended, and counted, one dropped step per batch row."""
    _each(_random_case_both_forms, ops, RANDOM)
    _each(_one_launch_equals_write_then_two_launches, ops, SHAPES)
    _each(_slot_outside_the_cache, ops, ((-1,), (700,)))
