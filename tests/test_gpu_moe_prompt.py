"""The device-side prompt path of the routed W8A16 experts: eetq_w8a16_moe_gemm_tiled against the oracle and against
the forced tiled GEMM on every expert's gathered rows (bit for bit), placement independence, untouched rows, the layer at T > 16
against float32 on the dequantised stacks, graph capture of the forward and of forward + backward at T = 64 (the proof that no
launch of the default route reads anything back to the host), trainable forward == inference forward and gradients on a shape
the tiled kernel serves, and tiny Mixtral / Qwen3-MoE models on a 40-token prompt."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_moe import _close, _experts, _glu8, _route, _router_weights, _routing, _silu_mul_np, _stack, _tier_a, _tiny
from test_gpu_moe_backward import _ref_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_UNSUPPORTED = -3
TILED = (8, 512, 1024, 2)     # E, H, I, k: both projections inside the tile body's limits (K = 512 and 1024 >= 320)
TINY = [(8, 256, 128, 2), (128, 128, 64, 8)]   # the existing layer tests' shapes (K < 320: the decode kernel serves them)


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    L = _lib.lib()
    assert L.eetq_device_supported() == 1, "kernels are built for gfx950 only"
    return L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _prompt_routing(T, k, E, kind, seed):
    if kind != "straddle":
        return _routing(T, k, E, kind, seed)
    # k = 1: counts 127, 128, 129 and 1 on experts 0, 2, 3, 5 (T = 385), in shuffled token order
    assert k == 1 and T == 385 and E >= 6
    ids = torch.tensor([0] * 127 + [2] * 128 + [3] * 129 + [5])
    g = torch.Generator().manual_seed(seed)
    return ids[torch.randperm(T, generator=g)].reshape(T, 1).to(DEV)


CASES = [(300, 2, 8, "uniform"), (300, 2, 8, "one"), (200, 1, 8, "few"), (130, 2, 8, "sentinel"), (150, 2, 8, "dup"),
         (64, 8, 128, "uniform"), (385, 1, 8, "straddle")]


@pytest.mark.parametrize("K", [768, 2048, 4096])
@pytest.mark.parametrize("T,k,E,kind", CASES)
def test_tiled_entry_against_oracle_and_forced_tile_path(lib, K, T, k, E, kind):
    import oracle
    from eetq_amd.ops import w8_a16_gemm
    N = 320   # not a multiple of the 128- or 64-column tiles
    raw, processed, scales = _stack(E, K, N, seed=K + T)
    gproc, gscales = _glu8(processed, scales, K)
    x = (torch.rand(T, K) - 0.5).half()
    idx = _prompt_routing(T, k, E, kind, seed=K)
    counts, offsets, sorted_slot, position, active = _route(lib, idx, E)
    S = T * k
    used = int(offsets[-1])
    xd = x.to(DEV)
    POISON = -777.0
    plain = torch.full((S, N), POISON, dtype=torch.float16, device=DEV)
    glu = torch.full((S, N // 2), POISON, dtype=torch.float16, device=DEV)
    contig = torch.full((S, N), POISON, dtype=torch.float16, device=DEV)
    gplain = torch.full((S, N), POISON, dtype=torch.float16, device=DEV)
    args = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
    f = lib.eetq_w8a16_moe_gemm_tiled
    assert f(_ptr(xd), _ptr(processed), _ptr(scales), *args, _ptr(plain), T, k, E, N, K, 1, 0, _stream()) == 0
    assert f(_ptr(xd), _ptr(gproc), _ptr(gscales), *args, _ptr(glu), T, k, E, N, K, 1, 1, _stream()) == 0
    # the contiguous form reads the gathered rows in sorted order (rows past offsets[E]: NaN, which nothing may read into a live row)
    sorted_h = torch.cat([x[sorted_slot[:used].long().cpu() // k],
                          torch.full((S - used, K), float("nan"), dtype=torch.float16)]).to(DEV)
    assert f(_ptr(sorted_h), _ptr(processed), _ptr(scales), *args, _ptr(contig), T, k, E, N, K, 0, 0, _stream()) == 0
    # the gated write-out == the plain projection of the glu8-ordered stack followed by eetq_silu_mul_glu8_f16, bit for bit
    assert f(_ptr(xd), _ptr(gproc), _ptr(gscales), *args, _ptr(gplain), T, k, E, N, K, 1, 0, _stream()) == 0
    gsep = torch.empty(S, N // 2, dtype=torch.float16, device=DEV)
    assert lib.eetq_silu_mul_glu8_f16(_ptr(gplain), _ptr(gsep), S, N // 2, _stream()) == 0
    # the decode kernel on the same tables: another summation order, the same contract
    dec = torch.full((S, N), POISON, dtype=torch.float16, device=DEV)
    assert lib.eetq_w8a16_moe_gemm(_ptr(xd), _ptr(processed), _ptr(scales), *args, _ptr(dec), T, k, E, N, K, 1, 0, _stream()) == 0
    torch.cuda.synchronize()
    off = offsets.cpu().numpy()
    slots = sorted_slot.cpu().numpy()
    s_np, raw_np = scales.cpu().numpy(), raw.numpy()
    seen = 0
    for e in range(E):
        c = off[e + 1] - off[e]
        if not c:
            continue
        seen += c
        rows = slice(off[e], off[e + 1])
        xe = x.numpy()[slots[rows] // k]
        ref = oracle.w8a16_gemm(xe, raw_np[e], s_np[e])
        assert _tier_a(plain[rows].cpu().numpy(), ref).all(), e
        assert torch.equal(contig[rows], plain[rows]), e
        ref_glu = _silu_mul_np(ref[:, :N // 2], ref[:, N // 2:])
        assert _tier_a(glu[rows].cpu().numpy(), ref_glu).all(), e
        assert torch.equal(glu[rows], gsep[rows]), e
        assert _tier_a(dec[rows].cpu().numpy(), plain[rows].cpu().numpy()).all(), e
        # the reused tile body: the forced tiled GEMM on the gathered rows (one unsplit launch at these shapes), bit for bit
        mfma = w8_a16_gemm(torch.from_numpy(xe).to(DEV), processed[e], scales[e], "mfma")
        assert torch.equal(plain[rows], mfma), e
    assert seen == used == int((idx >= 0).logical_and(idx < E).sum())
    # rows at or past offsets[E] are never written
    for buf in (plain, glu, contig, gplain):
        assert bool((buf[used:] == POISON).all())
    if kind == "sentinel":
        assert used < S
    if kind in ("one", "dup"):
        assert int(counts.max()) > 256 and int(counts.max()) % 128 != 0   # several row tiles and a ragged last one
    if kind == "few":
        assert int((counts == 0).sum()) > 0
    if kind == "straddle":
        assert sorted(counts.cpu().tolist()) == [0, 0, 0, 0, 1, 127, 128, 129]


@pytest.mark.parametrize("gather,glu8", [(1, 0), (1, 1), (0, 0)])
def test_k_below_the_ring_minimum_is_quietly_unsupported(lib, gather, glu8):
    T, k, E, N, K = 64, 2, 8, 256, 256   # K / 64 = 4 < 5 stages in flight
    _, processed, scales = _stack(E, K, N, seed=1)
    idx = _routing(T, k, E, "uniform", seed=1)
    _, offsets, sorted_slot, _, active = _route(lib, idx, E)
    x = torch.zeros(T * k, K, dtype=torch.float16, device=DEV)
    y = torch.full((T * k, N), -777.0, dtype=torch.float16, device=DEV)
    rc = lib.eetq_w8a16_moe_gemm_tiled(_ptr(x), _ptr(processed), _ptr(scales), _ptr(offsets), _ptr(sorted_slot), _ptr(active), _ptr(y),
                                       T, k, E, N, K, gather, glu8, _stream())
    assert rc == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == -777.0).all())   # nothing was launched


def test_entry_placement_independence(lib):
    """one (token row, expert) pair under two routings and two T: the same result bits wherever the row lands"""
    K, N, E, k = 1024, 256, 8, 2
    _, processed, scales = _stack(E, K, N, seed=3)
    g = torch.Generator().manual_seed(5)
    row = (torch.rand(K, generator=g) - 0.5).half()
    got = []
    for T, t, kind, seed in ((200, 7, "uniform", 1), (1000, 901, "one", 2), (77, 76, "dup", 3), (200, 7, "few", 4)):
        x = (torch.rand(T, K, generator=g) - 0.5).half()
        x[t] = row
        idx = _routing(T, k, E, kind, seed)
        idx[t, 0], idx[t, 1] = 4, 6
        _, offsets, sorted_slot, position, active = _route(lib, idx, E)
        y = torch.empty(T * k, N, dtype=torch.float16, device=DEV)
        assert lib.eetq_w8a16_moe_gemm_tiled(_ptr(x.to(DEV)), _ptr(processed), _ptr(scales), _ptr(offsets), _ptr(sorted_slot),
                                             _ptr(active), _ptr(y), T, k, E, N, K, 1, 0, _stream()) == 0
        pos = position.view(T, k)[t].long()
        got.append(y[pos].clone())
    torch.cuda.synchronize()
    assert len({int(p) for p in pos}) == 2
    for other in got[1:]:
        assert torch.equal(other, got[0])


def test_layer_placement_independence():
    """a token's output row is the same bits at two T served by the same grouped kernel, whatever the other tokens do"""
    E, H, I, k = TILED
    _, q, _ = _experts(E, H, I, k, seed=21)
    g = torch.Generator().manual_seed(6)
    row = torch.randn(H, generator=g).half()
    w = torch.tensor([0.7, 0.3])
    got = []
    for T, t, kind in ((64, 3, "uniform"), (300, 250, "one"), (2048, 1999, "sentinel")):   # S / E = 16, 75, 512: the tiled kernel
        x = torch.randn(T, H, generator=g).half()
        x[t] = row
        idx = _routing(T, k, E, kind, seed=T)
        idx[t, 0], idx[t, 1] = 2, 5
        wts = _router_weights(T, k, seed=T)
        wts[t] = w.to(DEV)
        got.append(q(x.to(DEV), idx, wts)[t].clone())
    for other in got[1:]:
        assert torch.equal(other, got[0])


def _layer_ref(x, idx, wts, deq, E):
    """float32 layer on the dequantised weights, one expert at a time (test_gpu_moe._layer_ref without its [S, H, 2I] gather)"""
    gu, dn = deq
    I = dn.shape[1]
    T, k = idx.shape
    contrib = torch.zeros(T * k, x.shape[1], dtype=torch.float32, device=DEV)
    ids = idx.flatten()
    for e in range(E):
        sl = (ids == e).nonzero().flatten()
        if not sl.numel():
            continue
        h = x.float()[sl // k] @ gu[e].float()
        a = torch.nn.functional.silu(h[:, :I]) * h[:, I:]
        contrib[sl] = (a @ dn[e].float()) * wts.flatten().float()[sl, None]
    out = torch.zeros(x.shape, dtype=torch.float32, device=DEV)
    for j in range(k):   # slot order within each token, as the combine adds
        out += contrib.view(T, k, -1)[:, j]
    return out


@pytest.mark.parametrize("E,H,I,k", TINY + [TILED])
@pytest.mark.parametrize("T", [17, 64, 300, 2048])
@pytest.mark.parametrize("kind", ["uniform", "one", "few", "sentinel", "dup"])
def test_layer_against_fp32_reference(lib, E, H, I, k, T, kind):
    from eetq_amd.ops import w8_a16_moe_train
    _, q, deq = _experts(E, H, I, k, seed=E + H)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, kind, seed=T)
    wts = _router_weights(T, k, seed=T + 1)
    y = q(x, idx, wts)
    assert y.shape == (T, H) and y.dtype == torch.float16
    ref = _layer_ref(x, idx, wts, deq, E)
    assert ref.abs().max() > 0.5
    assert _close(y, ref), (y.float() - ref).abs().max().item()
    assert torch.equal(q(x, idx, wts), y)   # deterministic call to call
    assert not _close(torch.zeros_like(ref), ref)
    if kind != "dup":   # the bound has teeth: reversed router weights fail it
        assert not _close(_layer_ref(x, idx, wts.flip(-1), deq, E), ref)
    # the trainable forward returns the same bits
    out, _, _, _ = w8_a16_moe_train(x, idx, wts, q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)
    assert torch.equal(out, y)


@pytest.mark.parametrize("E,H,I,k", [TINY[0], TILED])
def test_forward_is_captured_at_t64_and_replays_rewritten_routing(E, H, I, k):
    """capture is the proof of "no host read-back": a .cpu() of the expert counts is illegal while a stream is capturing"""
    _, q, _ = _experts(E, H, I, k, seed=9)
    T = 64
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "uniform", seed=1)
    wts = _router_weights(T, k, seed=2)
    assert torch.equal(q(x, idx, wts), q(x, idx, wts))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        q(x, idx, wts)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = q(x, idx, wts)
    for seed, kind in ((2, "uniform"), (3, "sentinel"), (4, "one"), (5, "dup")):
        idx.copy_(_routing(T, k, E, kind, seed=seed))
        wts.copy_(_router_weights(T, k, seed=seed))
        x.copy_(torch.randn(T, H, device=DEV).half())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, q(x, idx, wts)), kind


@pytest.mark.parametrize("E,H,I,k", [TINY[0], TILED])
def test_train_forward_and_backward_are_captured_at_t64(E, H, I, k):
    from eetq_amd.ops import w8_a16_moe_backward, w8_a16_moe_train
    _, q, _ = _experts(E, H, I, k, seed=2)
    T = 64
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "sentinel", seed=5)
    wts = _router_weights(T, k, seed=6)
    dout = torch.randn(T, H, device=DEV).half()
    stacks = (q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)

    def fresh():
        out, tables, gate_up, y = w8_a16_moe_train(x, idx, wts, *stacks)
        gx, gw = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
        return out, gx, gw

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fresh()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = fresh()
    for seed, kind in ((7, "uniform"), (8, "one"), (9, "sentinel")):
        idx.copy_(_routing(T, k, E, kind, seed=seed))
        wts.copy_(_router_weights(T, k, seed=seed))
        x.copy_(torch.randn(T, H, device=DEV).half())
        dout.copy_(torch.randn(T, H, device=DEV).half())
        g.replay()
        torch.cuda.synchronize()
        for a, b, name in zip(cap, fresh(), ("out", "grad_hidden", "grad_weights")):
            assert torch.equal(a, b), (kind, name)
        assert torch.equal(cap[0], q(x, idx, wts)), kind   # and the inference forward's bits


@pytest.mark.parametrize("T", [64, 300])
@pytest.mark.parametrize("kind", ["uniform", "sentinel", "one"])
def test_trainable_forward_and_gradients_on_the_tiled_shape(T, kind):
    E, H, I, k = TILED
    _, q, deq = _experts(E, H, I, k, seed=11)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, kind, seed=T)
    wts = _router_weights(T, k, seed=T)
    with torch.no_grad():
        want = q(x, idx, wts)
    q.trainable = True
    xg, wg = x.clone().requires_grad_(), wts.clone().requires_grad_()
    got = q(xg, idx, wg)
    assert got.grad_fn is not None and torch.equal(got, want)
    G = torch.randn(T, H, device=DEV)
    (got.float() * G).sum().backward()
    gx, gw = _ref_grads(x, idx, wts, deq, E, G)
    assert gx.abs().max() > 0.1
    assert _close(xg.grad, gx), (xg.grad.float() - gx).abs().max().item()
    assert _close(wg.grad, gw), (wg.grad.float() - gw).abs().max().item()
    assert not _close(torch.zeros_like(gx), gx)


@pytest.mark.parametrize("which", ["mixtral", "qwen3_moe"])
def test_tiny_models_on_a_40_token_prompt(which):
    from eetq_amd.modules.qlinear import W8A16Experts
    from eetq_amd.ops import quant_weights
    from eetq_amd.utils.quantizer import eet_quantize
    model = _tiny(which)
    ref = copy.deepcopy(model)
    eet_quantize(model, experts=True)
    eet_quantize(ref)  # same attention projections; experts stay fp16 -- set to the dequantised int8 weights below
    with torch.no_grad():
        for layer in ref.model.layers:
            ex = layer.mlp.experts
            for p in (ex.gate_up_proj, ex.down_proj):
                raw, _, s = quant_weights(p.transpose(1, 2).contiguous(), torch.int8, True)
                p.copy_((raw.float() * s.float()[:, None, :]).half().transpose(1, 2))
    assert all(isinstance(layer.mlp.experts, W8A16Experts) for layer in model.model.layers)
    ids = torch.randint(0, 512, (1, 40), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        got = model(ids).logits.float()
        want = ref(ids).logits.float()
    assert np.isfinite(got.cpu().numpy()).all()
    assert (got - want).abs().max() <= 2e-2 * want.abs().max()
