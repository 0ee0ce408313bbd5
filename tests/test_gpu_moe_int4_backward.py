"""Backward of the routed W4A16 experts layer: the grouped int4 input-gradient GEMM against w4_a16_gemm_t per expert
and against the int8 grouped kernel on the same integers (bit for bit), exact hot rows against the oracle's unpacked integers, the
trainable forward against the inference forward on every path (bit for bit), the layer's gradients against float32 autograd on the
dequantised int4 stacks, the whole backward against the int8 backward on the expanded stacks (bit for bit), replay, graph capture
and memory, and end-to-end gradients of tiny Mixtral / Qwen3-MoE models after eet_quantize(expert_bits=4) +
set_trainable(int4_experts=True).

The shapes are the smallest that reach every way the kernel can go wrong: H and I multiples of 128 (the int4 layout's floor), several
experts (a wrong expert stride), an expert with more than 128 rows (a second row tile of one expert: "one" at T = 300), empty
experts ("few"), sentinel and duplicate slots, T on both sides of 16.  Tolerance where one is used: test_gpu_moe._close, the
project's bound for gradients against float32, unchanged."""
import ctypes

import numpy as np
import pytest
import torch
import torch.utils.checkpoint

from test_gpu_moe import _close, _route, _router_weights, _routing
from test_gpu_moe_backward import _ref_grads, _silu_without_its_derivative_term
from test_gpu_moe_int4 import _experts4, _module_values, _tiny4

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["uniform", "one", "few", "sentinel", "dup"]
POISON = -777.0


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


_STACKS, _EXPANDED, _MODULES = {}, {}, {}


def _random_stack4(E, K, N):
    """random bytes as an int4 stack [E, K, N / 2] (every byte is two valid nibbles) and small fp16 scales [E, N], cached"""
    if (E, K, N) not in _STACKS:
        g = torch.Generator(device=DEV).manual_seed(E * 7 + K + N)
        w = torch.randint(-128, 128, (E, K, N // 2), dtype=torch.int8, device=DEV, generator=g)
        s = (torch.rand(E, N, device=DEV, generator=g) * 2e-2 + 1e-3).half()
        _STACKS[(E, K, N)] = (w, s)
    return _STACKS[(E, K, N)]


def _expand(lib, w4):
    """the int8 stack [E, K, N] holding the integers of the int4 stack w4 [E, K, N / 2] (eetq_expand_i4_to_i8), cached per tensor"""
    key = w4.data_ptr()
    if key not in _EXPANDED:
        E, K, n2 = w4.shape
        w8 = torch.empty(E, K, 2 * n2, dtype=torch.int8, device=DEV)
        assert lib.eetq_expand_i4_to_i8(_ptr(w4), _ptr(w8), w4.numel(), _stream()) == 0
        _EXPANDED[key] = (w4, w8)   # w4 kept alive: its address is the key
    return _EXPANDED[key][1]


def _module(E, H, I, k):
    """a W4A16Experts and the fp16(q s) stacks of its integers in [gate | up] order: ([E, H, 2I], [E, I, H]), through the oracle"""
    if (E, H, I, k) not in _MODULES:
        _, q = _experts4(E, H, I, k, seed=E + H)
        gu_q, gu_s, dn_q, dn_s = _module_values(q)
        gu = (gu_q.astype(np.float32) * gu_s.astype(np.float32)[:, None, :]).astype(np.float16)   # glu8 order
        v = gu.reshape(E, H, 2 * I // 16, 2, 8)
        gu = np.concatenate([v[:, :, :, 0].reshape(E, H, I), v[:, :, :, 1].reshape(E, H, I)], -1)
        dn = (dn_q.astype(np.float32) * dn_s.astype(np.float32)[:, None, :]).astype(np.float16)
        _MODULES[(E, H, I, k)] = (q, (torch.from_numpy(gu).to(DEV), torch.from_numpy(dn).to(DEV)))
    return _MODULES[(E, H, I, k)]


def _stacks(q):
    return (q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)


def _grouped(lib, fn, dy, w, s, offsets, active, T, k, E, N, K):
    dx = torch.full((T * k, K), POISON, dtype=torch.float16, device=DEV)   # rows past offsets[E] must stay as they are
    assert fn(_ptr(dy), _ptr(w), _ptr(s), _ptr(offsets), _ptr(active), _ptr(dx), T, k, E, N, K, _stream()) == 0
    return dx


# ---- 1. grouped int4 gemm_t == w4_a16_gemm_t on every expert's rows, bit for bit ---------------------------------------------
@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 128, 8), (8, 512, 384, 2)])
@pytest.mark.parametrize("T", [1, 5, 16, 17, 300])
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_gemm_t_equals_per_expert_gemm_t(lib, E, H, I, k, T, kind):
    from eetq_amd.ops import w4_a16_gemm_t
    S = T * k
    idx = _routing(T, k, E, kind, seed=T + E)
    counts, offsets, _, _, active = _route(lib, idx, E)
    used = int(offsets[-1])
    off = offsets.cpu().tolist()
    for K, N in ((I, H), (H, 2 * I)):   # the down stack and the gate|up stack
        w, s = _random_stack4(E, K, N)
        dy = torch.randn(S, N, device=DEV).half()
        dx = _grouped(lib, lib.eetq_w4a16_moe_gemm_t, dy, w, s, offsets, active, T, k, E, N, K)
        for e in range(E):
            if off[e + 1] == off[e]:
                continue
            rows = slice(off[e], off[e + 1])
            assert torch.equal(dx[rows], w4_a16_gemm_t(dy[rows], w[e], s[e])), (e, K, N)
        assert bool((dx[used:] == POISON).all())
        assert used == 0 or float(dx[:used].float().abs().max()) > 0.5
    if kind == "one" and T == 300:
        assert int(counts.max()) > 128   # an expert with a second row tile
    if kind == "few":
        assert int((counts == 0).sum()) > 0


# ---- 2. exact hot rows --------------------------------------------------------------------------------------------------------
def test_hot_rows_are_the_oracles_dequantised_integers(lib):
    """one sorted row per (expert e, column n) with dy one-hot at n: dx[k] = fp16(fp16(q[e, k, n]) * s[e, n]) exactly -- a wrong
    expert base, nibble position or scale row shows in some (e, n)"""
    import oracle
    from eetq_amd.ops import quant_weights
    E, K, N = 4, 256, 128
    torch.manual_seed(4)
    _, proc, scales = quant_weights((torch.randn(E, K, N) * 0.05).half(), torch.quint4x2, True)
    q = np.stack([oracle.i4_values(oracle.gfx950_unpack_i4(t)) for t in proc.numpy()])   # [E, K, N], -8 .. 7
    assert q.min() == -8 and q.max() == 7
    T, k = E * N, 1
    idx = (torch.arange(T) // N).reshape(T, 1).to(DEV)          # token t -> expert t / N: sorted row p = t (stable)
    _, offsets, sorted_slot, _, active = _route(lib, idx, E)
    assert offsets.cpu().tolist() == [N * e for e in range(E + 1)] and sorted_slot.cpu().tolist() == list(range(T))
    dy = torch.zeros(T, N, dtype=torch.float16, device=DEV)
    dy[torch.arange(T), torch.arange(T) % N] = 1.0
    dx = _grouped(lib, lib.eetq_w4a16_moe_gemm_t, dy, proc.to(DEV), scales.to(DEV), offsets, active, T, k, E, N, K)
    want = (q.astype(np.float32) * scales.numpy().astype(np.float32)[:, None, :]).astype(np.float16)   # one rounding: the product is exact in fp32
    want = np.ascontiguousarray(want.transpose(0, 2, 1)).reshape(T, K)                                 # row e N + n = column n of expert e
    assert np.array_equal(dx.cpu().numpy(), want)
    assert len({want[e * N:(e + 1) * N].tobytes() for e in range(E)}) == E


# ---- 3. the same bits as the int8 grouped kernel on the same integers ---------------------------------------------------------
@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 128, 8), (8, 512, 384, 2)])
@pytest.mark.parametrize("T,kind", [(5, "sentinel"), (17, "few"), (300, "one"), (300, "dup")])
def test_grouped_gemm_t_equals_the_int8_kernel_on_the_expanded_stack(lib, E, H, I, k, T, kind):
    idx = _routing(T, k, E, kind, seed=T + E)
    _, offsets, _, _, active = _route(lib, idx, E)
    for K, N in ((I, H), (H, 2 * I)):
        w, s = _random_stack4(E, K, N)
        dy = torch.randn(T * k, N, device=DEV).half()
        got = _grouped(lib, lib.eetq_w4a16_moe_gemm_t, dy, w, s, offsets, active, T, k, E, N, K)
        want = _grouped(lib, lib.eetq_w8a16_moe_gemm_t, dy, _expand(lib, w), s, offsets, active, T, k, E, N, K)
        assert torch.equal(got, want), (K, N)


# ---- 4. trainable forward == inference forward; who gets a grad_fn ------------------------------------------------------------
def _check_train_forward(q, E, H, I, k, T, path):
    from eetq_amd.ops import w4_a16_moe, w4_a16_moe_train
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "sentinel", seed=T)
    wts = _router_weights(T, k, seed=T)
    want = w4_a16_moe(x, idx, wts, *_stacks(q), path=path)
    out, tables, gate_up, y = w4_a16_moe_train(x, idx, wts, *_stacks(q), path=path)
    assert float(want.float().abs().max()) > 0.25
    assert torch.equal(out, want)
    S = T * k
    assert tables.dtype == torch.int32 and tables.shape == (2 * E + 1 + 2 * S + min(E, S),)
    assert gate_up.dtype == torch.float16 and gate_up.shape == (S, 2 * I)
    assert y.dtype == torch.float16 and y.shape == (S, H)
    return x, idx, wts, want


@pytest.mark.parametrize("path", ["auto", "decode"])
@pytest.mark.parametrize("T", [1, 16, 17, 100])
@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 128, 8)])
def test_trainable_forward_is_the_inference_forward(E, H, I, k, T, path):
    q, _ = _module(E, H, I, k)
    x, idx, wts, want = _check_train_forward(q, E, H, I, k, T, path)
    if path != "auto":
        return
    assert q.trainable is False
    xg, wg = x.clone().requires_grad_(), wts.clone().requires_grad_()
    try:
        got = q(xg, idx, wg)
        assert got.grad_fn is None and torch.equal(got, want)     # default: inference only, as before
        q.trainable = True
        got = q(xg, idx, wg)
        assert got.grad_fn is not None and torch.equal(got, want)
        assert torch.equal(q(x, idx, wg), want) and q(x, idx, wg).grad_fn is not None
        assert torch.equal(q(xg, idx, wts), want) and q(xg, idx, wts).grad_fn is not None
        assert q(x, idx, wts).grad_fn is None                      # nothing requires grad
        with torch.no_grad():
            assert q(xg, idx, wg).grad_fn is None
    finally:
        q.trainable = False


@pytest.mark.parametrize("path", ["expand", "direct"])
def test_trainable_forward_on_the_tiled_paths(path):
    """(8, 384, 384, 2), T = 64: a shape both tiled kernels take; the module's prompt_path reaches the Function"""
    from eetq_amd.ops import w4_a16_moe_direct_supported
    E, H, I, k, T = 8, 384, 384, 2, 64
    assert w4_a16_moe_direct_supported(T, k, E, H, I)
    q, _ = _module(E, H, I, k)
    x, idx, wts, want = _check_train_forward(q, E, H, I, k, T, path)
    if path == "direct":
        try:
            q.prompt_path, q.trainable = "direct", True
            assert q.op_path(T, k) == "direct"
            got = q(x.clone().requires_grad_(), idx, wts)
            assert got.grad_fn is not None and torch.equal(got, want)
        finally:
            q.prompt_path, q.trainable = "auto", False


# ---- 5. layer gradients against float32 autograd on the dequantised int4 stacks ----------------------------------------------
@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 128, 8)])
@pytest.mark.parametrize("T", [1, 3, 16, 17, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_layer_gradients_against_fp32_reference(E, H, I, k, T, kind):
    q, deq = _module(E, H, I, k)
    x = torch.randn(T, H, device=DEV).half().requires_grad_()
    idx = _routing(T, k, E, kind, seed=T)
    wts = _router_weights(T, k, seed=T + 1).requires_grad_()
    wts16 = wts.detach().half().requires_grad_()
    G = torch.randn(T, H, device=DEV)
    try:
        q.trainable = True
        (q(x, idx, wts).float() * G).sum().backward()
        x16 = x.detach().clone().requires_grad_()
        (q(x16, idx, wts16).float() * G).sum().backward()
    finally:
        q.trainable = False
    assert x.grad.dtype == torch.float16 and wts.grad.dtype == torch.float32
    assert x16.grad.dtype == torch.float16 and wts16.grad.dtype == torch.float16
    gx, gw = _ref_grads(x, idx, wts, deq, E, G)
    assert gx.abs().max() > 0.1
    assert _close(x.grad, gx), (x.grad.float() - gx).abs().max().item()
    assert _close(wts.grad, gw), (wts.grad.float() - gw).abs().max().item()
    gx16, gw16 = _ref_grads(x, idx, wts16.detach().float(), deq, E, G)
    assert _close(x16.grad, gx16) and _close(wts16.grad, gw16)
    # the bound has teeth: zero gradients, a missing silu' term and a dropped heaviest slot fail it
    assert not _close(torch.zeros_like(gx), gx) and not _close(torch.zeros_like(gw), gw)
    bad_x, _ = _ref_grads(x, idx, wts, deq, E, G, act=_silu_without_its_derivative_term)
    assert not _close(bad_x, gx)
    if kind != "dup":
        dropped = idx.clone()
        live = wts.detach().masked_fill((idx < 0) | (idx >= E), -1.0)
        dropped.scatter_(1, live.argmax(-1, keepdim=True), -1)
        dx_drop, dw_drop = _ref_grads(x, dropped, wts, deq, E, G)
        assert not (_close(dx_drop, gx) and _close(dw_drop, gw))


# ---- 6. the backward == the int8 backward on the same integers, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("E,H,I,k,T,kind", [(8, 256, 128, 2, 5, "sentinel"), (8, 256, 128, 2, 100, "one"), (128, 128, 128, 8, 17, "few"),
                                            (8, 512, 384, 2, 300, "dup")])
@pytest.mark.parametrize("wdtype", [torch.float32, torch.float16])
def test_backward_equals_the_int8_backward_on_the_expanded_stacks(lib, E, H, I, k, T, kind, wdtype):
    from eetq_amd.ops import w4_a16_moe_backward, w4_a16_moe_train, w8_a16_moe_backward
    q, _ = _module(E, H, I, k)
    gu_w, gu_s, dn_w, dn_s = _stacks(q)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, kind, seed=T)
    wts = _router_weights(T, k, seed=T + 1).to(wdtype)
    _, tables, gate_up, y = w4_a16_moe_train(x, idx, wts, gu_w, gu_s, dn_w, dn_s)
    dout = torch.randn(T, H, device=DEV).half()
    gx, gw = w4_a16_moe_backward(dout, wts, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s, True, True)
    wx, ww = w8_a16_moe_backward(dout, wts, tables, gate_up, y, _expand(lib, gu_w), gu_s, _expand(lib, dn_w), dn_s, True, True)
    assert gw.dtype == wdtype and float(gx.float().abs().max()) > 0.1
    assert torch.equal(gx, wx) and torch.equal(gw, ww)


# ---- 7. replay, graph capture, memory -----------------------------------------------------------------------------------------
def test_backward_replays_and_returns_only_what_is_asked():
    from eetq_amd.ops import w4_a16_moe_backward, w4_a16_moe_train
    E, H, I, k, T = 8, 256, 128, 2, 64
    q, _ = _module(E, H, I, k)
    stacks = _stacks(q)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "sentinel", seed=5)
    wts = _router_weights(T, k, seed=6)
    _, tables, gate_up, y = w4_a16_moe_train(x, idx, wts, *stacks)
    dout = torch.randn(T, H, device=DEV).half()
    a = w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
    b = w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    nx, nw = w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, False, True)
    assert nx is None and torch.equal(nw, a[1])
    nx, nw = w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, False)
    assert nw is None and torch.equal(nx, a[0])
    assert w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, False, False) == (None, None)
    # the saved tensors are only read: a retained graph runs the backward again and accumulates the same gradient
    xg, wg = x.clone().requires_grad_(), wts.clone().requires_grad_()
    try:
        q.trainable = True
        loss = (q(xg, idx, wg).float() * dout.float()).sum()
    finally:
        q.trainable = False
    loss.backward(retain_graph=True)
    once_x, once_w = xg.grad.clone(), wg.grad.clone()
    assert torch.equal(once_x, a[0]) and torch.equal(once_w, a[1])
    loss.backward()
    assert torch.equal(xg.grad, once_x + once_x) and torch.equal(wg.grad, once_w + once_w)


def test_trainable_forward_and_backward_in_one_graph():
    from eetq_amd.ops import w4_a16_moe_backward, w4_a16_moe_train
    E, H, I, k, T = 8, 256, 128, 2, 64
    q, _ = _module(E, H, I, k)
    stacks = _stacks(q)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "sentinel", seed=5)
    wts = _router_weights(T, k, seed=6)
    dout = torch.randn(T, H, device=DEV).half()

    def step():
        out, tables, gate_up, y = w4_a16_moe_train(x, idx, wts, *stacks)
        return (out,) + tuple(w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = step()
    for seed in (1, 2):
        dout.copy_(torch.randn(T, H, generator=torch.Generator().manual_seed(seed)).half())
        x.copy_(torch.randn(T, H, generator=torch.Generator().manual_seed(seed + 10)).half())
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, step()):
            assert torch.equal(got, want)


def test_backward_memory_is_activations_only():
    """DESIGN.md 4.11's bound, and next to it the allocation sequence itself.  The backward holds, beyond its inputs and gw: dy and
    dh, then dh and dgate_up, then dgate_up and the per-slot dx, then gx (dy, dh and dgate_up each released once consumed): a peak
    of 2 S (2I + max(H, I)) + 2 T H bytes plus the router gradient, the [T, k] ones and the allocator's 512-byte rounding of at
    most six live blocks (64 KiB covers them at this shape).  An expansion of either stack inside the backward -- 1.5 MiB for the
    down stack, 3 MiB for gate|up at this shape -- exceeds that while its GEMM runs."""
    from eetq_amd.ops import w4_a16_moe_backward, w4_a16_moe_train
    E, H, I, k, T = 8, 512, 384, 2, 300
    q, _ = _module(E, H, I, k)
    stacks = _stacks(q)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "uniform", seed=1)
    wts = _router_weights(T, k, seed=2)
    _, tables, gate_up, y = w4_a16_moe_train(x, idx, wts, *stacks)
    dout = torch.randn(T, H, device=DEV).half()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    gx, gw = w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    S = T * k
    bound = 2 * S * (3 * I + H) + 2 * T * H + (1 << 20)
    sequence = 2 * S * (2 * I + max(H, I)) + 2 * T * H + (64 << 10)     # the allocation sequence above
    print("peak %d bound %d sequence %d down stack as int8 %d" % (peak, bound, sequence, E * I * H))
    assert peak <= bound, (peak, bound)
    assert peak <= sequence, (peak, sequence)
    assert 2 * S * (H + I) + E * I * H > sequence                       # dy + dh + an expanded down stack would not fit
    assert torch.isfinite(gx.float()).all() and torch.isfinite(gw).all()


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------
def _reference_model(which, quantised):
    """the same model with every int4 experts module replaced by transformers' own experts holding the dequantised fp16 stacks:
    linears int8 and trainable as in the model under test, the experts' gradients torch's"""
    from eetq_amd.utils import eet_quantize
    ref = _tiny4(which)
    eet_quantize(ref, trainable=True)
    for layer, qlayer in zip(ref.model.layers, quantised.model.layers):
        qe, ex = qlayer.mlp.experts, layer.mlp.experts
        E, H, I = qe.num_experts, qe.hidden_dim, qe.intermediate_dim
        gu_q, gu_s, dn_q, dn_s = _module_values(qe)
        gu = (gu_q.astype(np.float32) * gu_s.astype(np.float32)[:, None, :]).astype(np.float16)
        v = gu.reshape(E, H, 2 * I // 16, 2, 8)
        gu = np.concatenate([v[:, :, :, 0].reshape(E, H, I), v[:, :, :, 1].reshape(E, H, I)], -1)
        dn = (dn_q.astype(np.float32) * dn_s.astype(np.float32)[:, None, :]).astype(np.float16)
        with torch.no_grad():
            ex.gate_up_proj.copy_(torch.from_numpy(gu).transpose(1, 2))
            ex.down_proj.copy_(torch.from_numpy(dn).transpose(1, 2))
    return ref


def _grads(model, emb, G):
    model.zero_grad(set_to_none=True)
    e = emb.detach().clone().requires_grad_()
    logits = model(inputs_embeds=e).logits
    (logits.float() * G).sum().backward()
    return e.grad, [layer.mlp.gate.weight.grad for layer in model.model.layers], logits.detach()


@pytest.mark.parametrize("which,router", [("mixtral", False), ("qwen3_moe", False), ("mixtral", True)])
def test_end_to_end_gradients(which, router):
    from eetq_amd.modules.qlinear import W4A16Experts
    from eetq_amd.utils import eet_quantize, set_trainable
    model = _tiny4(which)
    eet_quantize(model, experts=True, expert_bits=4, router=router)
    assert all(type(layer.mlp.experts) is W4A16Experts for layer in model.model.layers)
    ref = _reference_model(which, model)
    ids = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(3)).to(DEV)
    emb = model.model.embed_tokens(ids).detach()
    G = torch.randn(2, 12, 512, generator=torch.Generator().manual_seed(4)).to(DEV)
    ref_x, ref_r, _ = _grads(ref, emb, G)
    # the linears alone (the two-argument switch): the experts are cut out of the graph, so the gradients are not the model's
    n = set_trainable(model, True)
    off_x, off_r, off_logits = _grads(model, emb, G)
    assert not (_close(off_x, ref_x) and all(g is not None and _close(g, r) for g, r in zip(off_r, ref_r)))
    assert set_trainable(model, True, int4_experts=True) == n + 2
    got_x, got_r, logits = _grads(model, emb, G)
    assert torch.equal(logits, off_logits)                           # the untrainable experts' logits, bit for bit
    assert got_x is not None and ref_x.abs().max() > 0
    print("inputs_embeds: max err / max ref %.3g" % ((got_x.float() - ref_x.float()).abs().max().item() / ref_x.float().abs().max().item()))
    assert _close(got_x, ref_x), (got_x.float() - ref_x.float()).abs().max().item() / ref_x.float().abs().max().item()
    for g, r in zip(got_r, ref_r):
        assert r.abs().max() > 0 and g is not None
        print("router: max err / max ref %.3g" % ((g.float() - r.float()).abs().max().item() / r.float().abs().max().item()))
        assert _close(g, r), (g.float() - r.float()).abs().max().item() / r.float().abs().max().item()
    # one decoder layer under non-reentrant checkpointing: the same gradients, bit for bit (eager attention: its backward has no
    # atomics)
    model.set_attn_implementation("eager")
    layer = model.model.layers[0]
    h = torch.randn(1, 12, 128, device=DEV).half()
    pos = torch.arange(12, device=DEV)[None]
    cos_sin = model.model.rotary_emb(h, pos)

    def run(use_ckpt):
        model.zero_grad(set_to_none=True)
        hh = h.clone().requires_grad_()
        if use_ckpt:
            out = torch.utils.checkpoint.checkpoint(layer, hh, position_embeddings=cos_sin, position_ids=pos, use_reentrant=False)
        else:
            out = layer(hh, position_embeddings=cos_sin, position_ids=pos)
        (out.float() * G[:1, :, :128]).sum().backward()
        return hh.grad, layer.mlp.gate.weight.grad
    a, b = run(False), run(True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
