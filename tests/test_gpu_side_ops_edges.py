"""Edges of the side ops in eetq_amd/csrc/norm_rope.hip that the dense parity matrix does not reach.

  * rotary + KV-cache write: the SCALAR form (partial rotation, head sizes off the 16-channel grid, cache strides that are
    no multiple of 8) in its decode and prompt shapes, and scalar against vector form bit for bit;
  * the cos|sin table's upper bound: a position at or beyond the table's last row is treated like a negative one --
    nothing rotated, nothing written, counted once -- in the cache-write launch and the plain rotary ops (the one-launch
    decode step's kernel carries no such bound: INTEGRATION.md); the legacy C entries (no row count) keep their bits;
  * RMS-norm at the widths where its loops change trip count, on unaligned storage and on non-finite rows;
  * silu_mul on zeros, subnormals, the fp32 expf overflow threshold, infinities and NaN.

Rotary comparisons are array_equal: the arithmetic is fp16 op for op (oracle.rotary_neox_f16).  The RMS-norm criterion is
test_layernorm_forward's: no output more than one fp16 step from the oracle, fewer than 2 % of a case's elements differing."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KSENT, VSENT = 7.0, -3.0      # cache sentinels: an element that still holds them was not written


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as _ops
    from eetq_amd import _lib
    assert _lib.lib().eetq_device_supported() == 1, "kernels are built for gfx950 only"
    return _ops


def _table(rot, rows, dtype=torch.float16):
    inv = 1.0 / (10000 ** (torch.arange(0, rot, 2).float() / rot))
    fr = torch.einsum("i,j->ij", torch.arange(rows).float(), inv)
    return torch.cat([fr.cos(), fr.sin()], -1).to(dtype)


def _guarded_table(rot, R, dtype=torch.float16, front=0):
    """The R table rows as a contiguous view into a larger device tensor whose other rows (8 behind, `front` before) are NaN:
    a read past the table stays inside the allocation and shows as NaN.  Returns (device view, CPU table)."""
    t = _table(rot, R, dtype)
    big = torch.full((front + R + 8, rot), float("nan"), dtype=dtype, device=DEV)
    big[front: front + R] = t.to(DEV)
    view = big[front: front + R]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view, t


def _views(d, H, Hkv, D):
    """q / k / v views [B, T, heads, D] into a fused projection output d [B, T, (H + 2 Hkv) D]"""
    q = d[..., : H * D].unflatten(-1, (H, D))
    k = d[..., H * D: (H + Hkv) * D].unflatten(-1, (Hkv, D))
    v = d[..., (H + Hkv) * D:].unflatten(-1, (Hkv, D))
    return q, k, v


def _caches(B, Hkv, S, D, pad=0):
    """(kc, vc) views [B, Hkv, S, D] into sentinel-filled tensors whose rows are D + pad elements apart"""
    kc = torch.full((B, Hkv, S, D + pad), KSENT, dtype=torch.float16, device=DEV)
    vc = torch.full((B, Hkv, S, D + pad), VSENT, dtype=torch.float16, device=DEV)
    return kc[..., :D], vc[..., :D], kc, vc


def _check_rotary_write(oracle, qkv, got, pos, rows, table, kc_store, vc_store, H, Hkv, D):
    """qkv: the projection output before the call, got: after it (CPU [B, T, row]); pos [B, T]: table rows; rows [B, T]: the
    cache row each token must land in, -1 for a token the kernel must drop; table: CPU [R, rot]; kc_store / vc_store: the
    caches' whole storage [B, Hkv, S, D + pad].  Checks q (rotated channels against the oracle, the others and every dropped
    token unchanged), the k | v part of the projection, and the complete cache images -- written rows and sentinels."""
    B, T = pos.shape
    rot = table.shape[1]
    pos = np.asarray(pos, np.int64).reshape(-1)
    rows = np.asarray(rows, np.int64).reshape(-1)
    live = rows >= 0
    qkv2, got2 = qkv.reshape(B * T, -1), got.reshape(B * T, -1)
    q0 = qkv2[:, : H * D].reshape(B * T, H, D).numpy()
    k0 = qkv2[:, H * D: (H + Hkv) * D].reshape(B * T, Hkv, D).numpy()
    v0 = qkv2[:, (H + Hkv) * D:].reshape(B * T, Hkv, D).numpy()
    safe = np.where(live, pos, 0)           # the oracle has no bound check: dropped tokens are not taken from it
    qo, _ = oracle.rotary_neox_f16(safe, q0, q0.copy(), table.numpy(), D)
    ko, _ = oracle.rotary_neox_f16(safe, k0, k0.copy(), table.numpy(), D)
    gq = got2[:, : H * D].reshape(B * T, H, D).numpy()
    assert np.array_equal(gq[live][..., :rot], qo[live][..., :rot]), "q: rotated channels"
    assert np.array_equal(gq[live][..., rot:], q0[live][..., rot:]), "q: channels >= rot_dim must stay"
    assert np.array_equal(gq[~live], q0[~live]), "q of a dropped token must stay as it was"
    assert torch.equal(got2[:, H * D:], qkv2[:, H * D:]), "the k and v parts of the projection must stay"
    kimg = np.full(tuple(kc_store.shape), KSENT, np.float16)
    vimg = np.full(tuple(vc_store.shape), VSENT, np.float16)
    for i in np.nonzero(live)[0]:
        b, r = i // T, rows[i]
        kimg[b, :, r, :rot] = ko[i][:, :rot]
        kimg[b, :, r, rot:D] = k0[i][:, rot:]
        vimg[b, :, r, :D] = v0[i]
    assert np.array_equal(kc_store.cpu().numpy(), kimg), "k cache image (written rows, sentinels, padding)"
    assert np.array_equal(vc_store.cpu().numpy(), vimg), "v cache image (written rows, sentinels, padding)"


# ------------------------------------------------------------------------------------------------ scalar form, decode step

@pytest.mark.parametrize("slot_mode", ["positions", "shared", "per_row"])
@pytest.mark.parametrize("B,H,Hkv,D,rot,S", [(3, 4, 2, 64, 32, 24),     # partial rotation at a head size the modules use
                                             (2, 4, 4, 80, 32, 16),     # D % 16 == 0 but rot != D
                                             (2, 3, 1, 72, 72, 16),     # full rotation, D % 16 != 0, embed = 36
                                             (2, 20, 20, 64, 8, 8)])    # q 80, k 80, tail 1120, v 1280 items: > 512 threads
def test_scalar_cache_write_decode(ops, oracle, B, H, Hkv, D, rot, S, slot_mode):
    torch.manual_seed(D * 100 + rot + S)
    table = _table(rot, 40)
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * D).half()
    if slot_mode == "positions":
        pos = torch.randperm(S)[:B]                        # the cache row is the position
        slots, rows = None, pos.clone()
    elif slot_mode == "shared":
        pos = torch.randint(0, 40, (B,))
        slots, rows = torch.tensor([S - 3]), torch.full((B,), S - 3)
    else:
        pos = torch.randint(0, 40, (B,))
        rows = (torch.arange(B) * 2 + 1) % S
        rows = torch.where(rows == pos, (rows + 1) % S, rows)   # every row differs from its position
        slots = rows.clone()
    d = qkv.to(DEV)
    q, k, v = _views(d, H, Hkv, D)
    kc, vc, kcs, vcs = _caches(B, Hkv, S, D)
    ops.decode_dropped_steps(reset=True)
    ops.rotary_embedding_neox_kvcache(pos.to(DEV), q[:, 0], k[:, 0], v[:, 0], D, table.to(DEV), kc, vc,
                                      slots=None if slots is None else slots.to(DEV))
    assert ops.decode_dropped_steps(reset=True) == 0
    _check_rotary_write(oracle, qkv, d.cpu(), pos.reshape(B, 1).numpy(), rows.reshape(B, 1).numpy(), table, kcs, vcs, H, Hkv, D)


# ------------------------------------------------------------------------------------------------ scalar form, prompt

@pytest.mark.parametrize("base,dev_base", [(3, False), (3, True), (14, True)])
def test_scalar_cache_write_prompt(ops, oracle, base, dev_base):
    """first_row on the host, a device counter (read, not advanced), and a device counter two rows before the cache's end: the
    tokens that do not fit are skipped whole (q too) and counted."""
    B, T, H, Hkv, D, rot, S = 2, 5, 4, 2, 64, 32, 16
    torch.manual_seed(base * 2 + dev_base)
    table = _table(rot, 40)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D).half()
    pos = (torch.arange(T)[None, :] + torch.arange(B)[:, None] * 3 + 2).contiguous()   # positions != cache rows
    rows = base + torch.arange(T)[None, :].repeat(B, 1)
    rows = torch.where(rows < S, rows, torch.full_like(rows, -1))
    d = qkv.to(DEV)
    q, k, v = _views(d, H, Hkv, D)
    kc, vc, kcs, vcs = _caches(B, Hkv, S, D)
    counter = torch.tensor(base, dtype=torch.int64, device=DEV)
    ops.decode_dropped_steps(reset=True)
    if dev_base:
        ops.rotary_embedding_neox_kvcache_prefill(pos.to(DEV), q, k, v, D, table.to(DEV), kc, vc, first_row_dev=counter)
        assert int(counter) == base, "the counter is read, not advanced"
    else:
        ops.rotary_embedding_neox_kvcache_prefill(pos.to(DEV), q, k, v, D, table.to(DEV), kc, vc, first_row=base)
    assert ops.decode_dropped_steps(reset=True) == B * max(0, base + T - S)      # base 14: B * (T - 2)
    _check_rotary_write(oracle, qkv, d.cpu(), pos.numpy(), rows.numpy(), table, kcs, vcs, H, Hkv, D)


# ------------------------------------------------------------------------------------------------ scalar == vector, bit for bit

@pytest.mark.parametrize("T", [0, 5])
def test_scalar_and_vector_forms_give_the_same_bits(ops, oracle, T):
    """Dense caches take the 16-byte form; caches whose rows are D + 4 = 68 elements apart (no multiple of 8) take the scalar
    one.  The same q and the same cache images, and the four padding columns keep the sentinel.  T = 0: decode step;
    T = 5: prompt with first_row = 2."""
    B, H, Hkv, D, S = 3, 8, 2, 64, 24
    torch.manual_seed(40 + T)
    table = _table(D, 48)
    Tn = max(T, 1)
    qkv = torch.randn(B, Tn, (H + 2 * Hkv) * D).half()
    if T == 0:
        pos = torch.tensor([[5], [23], [0]])
        rows = pos.clone()
    else:
        pos = (torch.arange(T)[None, :] * 2 + torch.arange(B)[:, None] * 7 + 1).contiguous()
        rows = 2 + torch.arange(T)[None, :].repeat(B, 1)
    res = []
    for pad in (0, 4):
        d = qkv.to(DEV)
        q, k, v = _views(d, H, Hkv, D)
        kc, vc, kcs, vcs = _caches(B, Hkv, S, D, pad)
        assert kc.stride(2) == D + pad
        if T == 0:
            ops.rotary_embedding_neox_kvcache(pos.reshape(-1).to(DEV), q[:, 0], k[:, 0], v[:, 0], D, table.to(DEV), kc, vc)
        else:
            ops.rotary_embedding_neox_kvcache_prefill(pos.to(DEV), q, k, v, D, table.to(DEV), kc, vc, first_row=2)
        _check_rotary_write(oracle, qkv, d.cpu(), pos.numpy(), rows.numpy(), table, kcs, vcs, H, Hkv, D)
        if pad:
            assert (kcs[..., D:] == KSENT).all() and (vcs[..., D:] == VSENT).all()
        res.append((d.clone(), kc.clone(), vc.clone()))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the table's upper bound

R = 16    # table rows of every bound test


@pytest.mark.parametrize("rot", [64, 32])     # vector form, scalar form
def test_table_bound_cache_write_decode(ops, oracle, rot):
    """positions [R - 1, R, R + 5, -1]: batch row 0 is rotated and cached; the others are dropped like a negative position --
    q as it was, nothing cached, three steps counted.  (Without the bound rows 1 and 2 read the NaN rows behind the table.)"""
    B, H, Hkv, D, S = 4, 4, 2, 64, 24
    torch.manual_seed(rot)
    tdev, table = _guarded_table(rot, R)
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * D).half()
    pos = torch.tensor([R - 1, R, R + 5, -1])
    rows = np.array([[R - 1], [-1], [-1], [-1]])
    d = qkv.to(DEV)
    q, k, v = _views(d, H, Hkv, D)
    kc, vc, kcs, vcs = _caches(B, Hkv, S, D)
    ops.decode_dropped_steps(reset=True)
    ops.rotary_embedding_neox_kvcache(pos.to(DEV), q[:, 0], k[:, 0], v[:, 0], D, tdev, kc, vc)
    dropped = ops.decode_dropped_steps(reset=True)
    _check_rotary_write(oracle, qkv, d.cpu(), pos.reshape(B, 1).numpy(), rows, table, kcs, vcs, H, Hkv, D)
    assert dropped == 3


@pytest.mark.parametrize("rot", [64, 32])
def test_table_bound_cache_write_prompt(ops, oracle, rot):
    B, T, H, Hkv, D, S = 2, 2, 4, 2, 64, 8
    torch.manual_seed(rot + 1)
    tdev, table = _guarded_table(rot, R)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D).half()
    pos = torch.tensor([[R - 1, R], [R + 5, -1]])
    rows = np.array([[1, -1], [-1, -1]])
    d = qkv.to(DEV)
    q, k, v = _views(d, H, Hkv, D)
    kc, vc, kcs, vcs = _caches(B, Hkv, S, D)
    ops.decode_dropped_steps(reset=True)
    ops.rotary_embedding_neox_kvcache_prefill(pos.to(DEV), q, k, v, D, tdev, kc, vc, first_row=1)
    dropped = ops.decode_dropped_steps(reset=True)
    _check_rotary_write(oracle, qkv, d.cpu(), pos.numpy(), rows, table, kcs, vcs, H, Hkv, D)
    assert dropped == 3


@pytest.mark.parametrize("kind,dtype,rot", [("plain", torch.float16, 64), ("plain", torch.float32, 64), ("plain", torch.float16, 32),
                                            ("strided", torch.float16, 64), ("strided", torch.float16, 32)])
def test_table_bound_plain_and_strided_rotary(ops, oracle, kind, dtype, rot):
    """Tokens at R and R + 5 come back unrotated, the others match the oracle, two are counted; then a negative position (a
    table with NaN rows in front of it as well): unrotated, one counted."""
    H, Hkv, D = 4, 2, 64
    torch.manual_seed(rot + (dtype == torch.float32))
    for front, positions, bad in ((0, [R - 1, R, R + 5, 3, 0], 2), (8, [2, -1, R - 1], 1)):
        tdev, table = _guarded_table(rot, R, dtype, front)
        pos = torch.tensor(positions)
        n = len(positions)
        live = ((pos >= 0) & (pos < R)).numpy()
        safe = np.where(live, pos.numpy(), 0)
        ops.decode_dropped_steps(reset=True)
        if kind == "plain":
            q0 = torch.randn(1, n, H, D).to(dtype)
            k0 = torch.randn(1, n, H, D).to(dtype)
            q, k = q0.to(DEV), k0.to(DEV)
            ops.rotary_embedding_neox(pos.reshape(1, n).to(DEV), q, k, D, tdev)
            qo, ko = oracle.rotary_neox(safe, q0.reshape(n, H, D).numpy(), k0.reshape(n, H, D).numpy(), table.numpy(), D)
            gq, gk = q.cpu().reshape(n, H, D).numpy(), k.cpu().reshape(n, H, D).numpy()
            q0, k0 = q0.reshape(n, H, D).numpy(), k0.reshape(n, H, D).numpy()
        else:
            qkv = torch.randn(1, n, (H + 2 * Hkv) * D).half()
            d = qkv.to(DEV)
            q, k, _ = _views(d, H, Hkv, D)
            ops.rotary_embedding_neox_strided(pos.to(DEV), q, k, D, tdev)
            q0 = qkv[0, :, : H * D].reshape(n, H, D).numpy()
            k0 = qkv[0, :, H * D: (H + Hkv) * D].reshape(n, Hkv, D).numpy()
            qo, _ = oracle.rotary_neox_f16(safe, q0, q0.copy(), table.numpy(), D)
            ko, _ = oracle.rotary_neox_f16(safe, k0, k0.copy(), table.numpy(), D)
            got = d.cpu()
            gq = got[0, :, : H * D].reshape(n, H, D).numpy()
            gk = got[0, :, H * D: (H + Hkv) * D].reshape(n, Hkv, D).numpy()
            assert torch.equal(got[..., (H + Hkv) * D:], qkv[..., (H + Hkv) * D:])
        dropped = ops.decode_dropped_steps(reset=True)
        assert np.array_equal(gq[live], qo[live]) and np.array_equal(gk[live], ko[live])
        assert np.array_equal(gq[~live], q0[~live]) and np.array_equal(gk[~live], k0[~live]), "out-of-table tokens stay unrotated"
        assert dropped == bad


def test_legacy_entries_keep_their_bits(ops, oracle):
    """The C entries that carry no table row count (eetq_rotary_neox_f16, eetq_rotary_neox, eetq_rotary_neox_strided_f16,
    eetq_rotary_neox_kvcache_f16, eetq_rotary_neox_kvcache_prefill_f16, eetq_rope_decode_attention_f16), called through
    ctypes with in-range positions: the oracle's bits, and for the one-launch step the bits of the bounded entry."""
    from eetq_amd import _lib
    L = _lib.lib()
    torch.manual_seed(77)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, T, H, Hkv, D, S = 2, 3, 4, 2, 64, 16
    n = B * T
    pos = torch.tensor([[3, 9, 15], [0, 7, 8]])
    pd = pos.to(DEV)
    for rot in (64, 32):
        table = _table(rot, R)
        tdev = table.to(DEV)
        # plain: fp16 entry, then the any-dtype entry in fp32
        q0, k0 = torch.randn(n, H, D).half(), torch.randn(n, H, D).half()
        q, k = q0.to(DEV), k0.to(DEV)
        _lib.check(L.eetq_rotary_neox_f16(vp(pd), vp(q), vp(k), vp(tdev), n, H, D, rot, stream))
        qo, ko = oracle.rotary_neox_f16(pos.numpy(), q0.numpy(), k0.numpy(), table.numpy(), D)
        assert np.array_equal(q.cpu().numpy(), qo) and np.array_equal(k.cpu().numpy(), ko)
        t32 = _table(rot, R, torch.float32)
        q0, k0 = torch.randn(n, H, D), torch.randn(n, H, D)
        q, k, t32d = q0.to(DEV), k0.to(DEV), t32.to(DEV)
        _lib.check(L.eetq_rotary_neox(vp(pd), vp(q), vp(k), vp(t32d), _lib.DTYPE_F32, n, H, D, rot, stream))
        qo, ko = oracle.rotary_neox(pos.numpy(), q0.numpy(), k0.numpy(), t32.numpy(), D)
        assert np.array_equal(q.cpu().numpy(), qo) and np.array_equal(k.cpu().numpy(), ko)
        # strided
        row = (H + 2 * Hkv) * D
        qkv = torch.randn(B, T, row).half()
        d = qkv.to(DEV)
        q, k, v = _views(d, H, Hkv, D)
        _lib.check(L.eetq_rotary_neox_strided_f16(vp(pd), vp(q), vp(k), vp(tdev), n, H, Hkv, D, rot, row, row, stream))
        q0 = qkv[..., : H * D].reshape(n, H, D).numpy()
        k0 = qkv[..., H * D: (H + Hkv) * D].reshape(n, Hkv, D).numpy()
        qo, _ = oracle.rotary_neox_f16(pos.numpy(), q0, q0.copy(), table.numpy(), D)
        ko, _ = oracle.rotary_neox_f16(pos.numpy(), k0, k0.copy(), table.numpy(), D)
        got = d.cpu()
        assert np.array_equal(got[..., : H * D].reshape(n, H, D).numpy(), qo)
        assert np.array_equal(got[..., H * D: (H + Hkv) * D].reshape(n, Hkv, D).numpy(), ko)
        # decode cache write (token 0 of every batch row), then the prompt form
        d = qkv[:, :1].contiguous().to(DEV)
        q, k, v = _views(d, H, Hkv, D)
        kc, vc, kcs, vcs = _caches(B, Hkv, S, D)
        st = (ctypes.c_long * 6)(row, row, row, kc.stride(0), kc.stride(1), kc.stride(2))
        p1 = pos[:, 0].contiguous()
        p1d = p1.to(DEV)
        _lib.check(L.eetq_rotary_neox_kvcache_f16(vp(p1d), None, 0, vp(q), vp(k), vp(v), vp(tdev), vp(kc), vp(vc), B, H, Hkv,
                                                  D, rot, st, S, stream))
        _check_rotary_write(oracle, qkv[:, :1], d.cpu(), p1.reshape(B, 1).numpy(), p1.reshape(B, 1).numpy(), table, kcs, vcs,
                            H, Hkv, D)
        d = qkv.to(DEV)
        q, k, v = _views(d, H, Hkv, D)
        kc, vc, kcs, vcs = _caches(B, Hkv, S, D)
        _lib.check(L.eetq_rotary_neox_kvcache_prefill_f16(vp(pd), vp(q), vp(k), vp(v), vp(tdev), vp(kc), vp(vc), B, T, None,
                                                          4, H, Hkv, D, rot, st, S, stream))
        rows = 4 + torch.arange(T)[None, :].repeat(B, 1)
        _check_rotary_write(oracle, qkv, d.cpu(), pos.numpy(), rows.numpy(), table, kcs, vcs, H, Hkv, D)
    # the one-launch step: legacy entry == bounded entry (through ops), same inputs
    table = _table(D, R).to(DEV)
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * D, dtype=torch.float16, device=DEV)
    q, k, v = (t[:, 0] for t in _views(qkv, H, Hkv, D))
    kc0 = torch.randn(B, Hkv, S, D, dtype=torch.float16, device=DEV)
    vc0 = torch.randn(B, Hkv, S, D, dtype=torch.float16, device=DEV)
    p1 = torch.tensor([R - 1, 4], device=DEV)
    slots = torch.tensor([5, 9], device=DEV)
    cnt = torch.tensor(10, dtype=torch.int64, device=DEV)
    tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)
    kc_a, vc_a, kc_b, vc_b = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
    out_a = ops.rope_decode_attention(p1, q, k, v, table, kc_a, vc_a, tickets, slots=slots, splits=2, kv_len=cnt)
    out_b = torch.empty_like(out_a)
    ws = torch.empty(B * H * 2 * (D + 4), dtype=torch.float32, device=DEV)
    st = (ctypes.c_long * 12)(q.stride(0), k.stride(0), v.stride(0), kc_b.stride(0), kc_b.stride(1), kc_b.stride(2), vc_b.stride(0),
                              vc_b.stride(1), vc_b.stride(2), 0, out_b.stride(0), out_b.stride(1))
    _lib.check(L.eetq_rope_decode_attention_f16(vp(p1), vp(slots), 1, vp(q), vp(k), vp(v), vp(table), vp(kc_b), vp(vc_b), None,
                                                vp(out_b), vp(ws), vp(tickets), B, H, Hkv, S, D, 2, D ** -0.5, st, vp(cnt), 0, None,
                                                stream))
    assert torch.equal(out_a, out_b) and torch.equal(kc_a, kc_b) and torch.equal(vc_a, vc_b)
    assert not torch.equal(kc_a, kc0) and torch.isfinite(out_a).all()


# ------------------------------------------------------------------------------------------------ RMS-norm

def _ordered(a):  # fp16 bit patterns (sign-magnitude) -> integers in value order
    i = np.ascontiguousarray(a).view(np.uint16).astype(np.int32)
    return np.where(i & 0x8000, -(i & 0x7FFF), i)


def _norm_criterion(got, ref):
    """test_layernorm_forward's: the fp32 sum of squares is the only order-dependent quantity, so no output is more than one fp16
    step from the oracle's (which sums in double), and fewer than 2 % of the elements differ at all."""
    gi, ri = _ordered(got), _ordered(ref)
    diff = np.abs(gi - ri)
    print("rmsnorm %s: max step %d, differing %.4f %%" % (got.shape, diff.max(), 100.0 * (gi != ri).mean()))
    assert diff.max() <= 1
    assert (gi != ri).mean() < 0.02


@pytest.mark.parametrize("rows,cols", [(2048, 1),      # scalar form, one active thread
                                       (300, 7),       # scalar form, width below 8
                                       (256, 8),       # vector form, one active lane
                                       (200, 9),       # scalar form
                                       (8, 257),       # scalar form, two trips for one thread
                                       (4, 1001),      # scalar form, four trips, ragged
                                       (3, 2056),      # vector form, second trip taken by one lane
                                       (2, 2049),      # scalar form, nine trips
                                       (2, 4100),      # scalar form
                                       (4100, 64)])    # more workgroups than one residency round
def test_rmsnorm_loop_edges(ops, oracle, rows, cols):
    torch.manual_seed(rows * 7 + cols)
    x = (torch.randn(rows, cols) * 3).half()
    g = (torch.rand(cols) + 0.5).half()
    out = torch.empty_like(x, device=DEV)
    ops.layernorm_forward(x.to(DEV), g.to(DEV), out, 1e-6)
    assert rows * cols >= 1800
    _norm_criterion(out.cpu().numpy(), oracle.rmsnorm_f16(x.numpy(), g.numpy(), 1e-6))


def test_rmsnorm_on_unaligned_storage(ops, oracle):
    """x, gamma and out as contiguous views 4 elements (8 bytes) into their storage, cols = 520 (a multiple of 8): the launcher
    must not issue 16-byte accesses there -- it takes the scalar form."""
    rows, cols = 28, 520
    torch.manual_seed(520)
    x = (torch.randn(rows, cols) * 3).half()
    g = (torch.rand(cols) + 0.5).half()
    n = rows * cols
    xb = torch.zeros(n + 8, dtype=torch.float16, device=DEV)
    gb = torch.zeros(cols + 8, dtype=torch.float16, device=DEV)
    ob = torch.full((n + 8,), 9.0, dtype=torch.float16, device=DEV)
    xv, gv, ov = xb[4: 4 + n].view(rows, cols), gb[4: 4 + cols], ob[4: 4 + n].view(rows, cols)
    xv.copy_(x)
    gv.copy_(g)
    assert xv.data_ptr() % 16 == 8 and gv.data_ptr() % 16 == 8 and ov.data_ptr() % 16 == 8
    ops.layernorm_forward(xv, gv, ov, 1e-6)
    _norm_criterion(ov.cpu().numpy(), oracle.rmsnorm_f16(x.numpy(), g.numpy(), 1e-6))
    assert (ob[:4] == 9.0).all() and (ob[4 + n:] == 9.0).all()


@pytest.mark.parametrize("cols", [64, 100])     # vector form, scalar form
@pytest.mark.parametrize("eps", [0.0, 1e-6])
def test_rmsnorm_non_finite_rows(ops, oracle, cols, eps):
    """Bit-exact against the oracle (nothing here depends on the summation order): a row with one +inf (scale 0: every finite
    element gives +-0, the inf gives NaN), a row with one NaN (every output NaN), an all-zero row (eps = 0: 0 * inf = NaN; eps > 0:
    zeros) and a row of +-65504 under gamma +-65000 (both clamp limits).  NaN leaves the clamp as -(65504 - 1000): the
    reference's max(NaN, -lim) == -lim, restated by the oracle."""
    torch.manual_seed(cols)
    x = (torch.randn(4, cols) * 3).half()
    x[0, cols // 3] = float("inf")
    x[1, cols - 1] = float("nan")
    x[2] = 0.0
    x[3] = 65504.0
    x[3, 1::3] = -65504.0
    g = torch.full((cols,), 65000.0).half()
    g[::2] = -65000.0
    out = torch.empty_like(x, device=DEV)
    ops.layernorm_forward(x.to(DEV), g.to(DEV), out, eps)
    got = out.cpu().numpy()
    ref = oracle.rmsnorm_f16(x.numpy(), g.numpy(), eps)
    assert np.array_equal(got.view(np.uint16), ref.view(np.uint16))
    # ... and the oracle says what the contract says
    lim = np.float16(-(65504.0 - 1000.0))
    assert got[0, cols // 3] == lim and np.all(got[0, np.arange(cols) != cols // 3] == 0)
    assert np.all(got[1] == lim)
    assert np.all(got[2] == lim) if eps == 0.0 else np.all(got[2] == 0)
    assert set(np.unique(got[3]).tolist()) == {float(lim), float(-lim)}


# ------------------------------------------------------------------------------------------------ silu_mul

def _silu_mul_reference(gate, up):
    """x / (1 + exp(-x)) in float64, rounded to fp32, rounded to fp16, then an fp16 multiply (numpy; -inf gives -inf / inf = NaN
    here as in the kernel)"""
    x = gate.astype(np.float64)
    with np.errstate(all="ignore"):
        s = (x / (1.0 + np.exp(-x))).astype(np.float32).astype(np.float16)
        return s * up, (x / (1.0 + np.exp(-x))).astype(np.float16) * up


def test_silu_mul_edge_values(ops):
    inf, nan = float("inf"), float("nan")
    gate_vals = [0.0, -0.0, 6e-8, -6e-8, 65504.0, -65504.0, -88.0, -89.0, -104.0, inf, -inf, nan,
                 65504.0, inf, -inf, 0.0, 1.0, -1.0, 3.5, -7.25, 0.1, -0.3, 11.0, -17.0, 2.0]
    up_vals = [1.0] * 12 + [-2.0, 0.0, 0.0, inf, -2.0, inf, 0.0] + [1.0] * 6
    I = 64
    gate = np.zeros((2, I), np.float16)
    up = np.ones((2, I), np.float16)
    gate[0, : len(gate_vals)] = gate_vals
    up[0, : len(up_vals)] = up_vals
    gate[0, len(gate_vals):] = np.linspace(-12, 12, I - len(gate_vals)).astype(np.float16)
    gate[1], up[1] = gate[0, ::-1], up[0, ::-1]               # the same pairs at other lanes
    ref, ref_direct = _silu_mul_reference(gate, up)
    # the reference's own double rounding (float64 -> fp32 -> fp16) moves no value by more than the step the kernel is allowed
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(ref), np.isnan(ref_direct)) and np.array_equal(np.isinf(ref), np.isinf(ref_direct))
    assert np.abs(_ordered(ref)[fin] - _ordered(ref_direct)[fin]).max() <= 1
    g, u = torch.from_numpy(gate), torch.from_numpy(up)
    plain = torch.cat([g, u], -1).to(DEV)                                              # [all gate | all up]
    glu8 = torch.stack([g.view(2, I // 8, 8), u.view(2, I // 8, 8)], 2).reshape(2, 2 * I).to(DEV)   # 8 gate + 8 up, repeated
    for out in (ops.silu_mul(plain), ops.silu_mul(glu8, glu8=True)):
        got = out.cpu().numpy()
        assert got.shape == (2, I)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN positions"
        assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]) and np.array_equal(np.isinf(got), np.isinf(ref))
        assert np.abs(_ordered(got)[fin] - _ordered(ref)[fin]).max() <= 1
    # what the listed values must give, whatever the reference says: -0 from the overflow side, NaN from -inf and from inf * 0
    got = ops.silu_mul(plain).cpu().numpy()[0]
    assert np.all(got[[0, 1, 5, 6, 7, 8]] == 0) and got[4] == 65504.0 and got[9] == inf
    assert np.isnan(got[[10, 11, 13, 14, 15]]).all() and got[12] == -inf
