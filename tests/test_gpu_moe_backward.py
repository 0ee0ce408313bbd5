"""Backward of the routed W8A16 experts layer: the grouped input-gradient GEMM against w8_a16_gemm_t per expert
(bit for bit), the gated-activation and combine backward kernels against torch, the layer's gradients against float32 autograd
on the dequantised stacks, the trainable forward against the inference forward (bit for bit), graph capture and determinism of
the backward, its memory, and end-to-end gradients of tiny Mixtral / Qwen3-MoE models after eet_quantize(trainable=True)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.utils.checkpoint

from test_gpu_moe import _close, _experts, _route, _router_weights, _routing, _tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["uniform", "one", "few", "sentinel", "dup"]


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


_STACKS = {}


def _random_stack(E, K, N):
    """random int8 bytes in the gfx950 layout [E, K, N] and small fp16 scales [E, N] (cached: the Mixtral stacks are 1.4 GB)"""
    if (E, K, N) not in _STACKS:
        g = torch.Generator(device=DEV).manual_seed(E * 7 + K + N)
        w = torch.randint(-127, 128, (E, K, N), dtype=torch.int8, device=DEV, generator=g)
        s = (torch.rand(E, N, device=DEV, generator=g) * 2e-3 + 1e-4).half()
        _STACKS[(E, K, N)] = (w, s)
    return _STACKS[(E, K, N)]


# ---- 1. grouped gemm_t == w8_a16_gemm_t on every expert's rows, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("E,H,I", [(8, 256, 192), (128, 128, 64), (8, 4096, 14336)])
@pytest.mark.parametrize("T", [1, 5, 16, 17, 300, 2048])
@pytest.mark.parametrize("kind", KINDS)
def test_grouped_gemm_t_equals_per_expert_gemm_t(lib, E, H, I, T, kind):
    from eetq_amd.ops import w8_a16_gemm_t
    k = 2 if E == 8 else 8
    S = T * k
    idx = _routing(T, k, E, kind, seed=T + E)
    counts, offsets, sorted_slot, position, active = _route(lib, idx, E)
    used = int(offsets[-1])
    off = offsets.cpu().tolist()
    # both directions of the layer: the down stack (N = H, K = I: K % 128 == 64 at I = 192) and the gate|up stack (N = 2I, K = H)
    for K, N in ((I, H), (H, 2 * I)):
        w, s = _random_stack(E, K, N)
        dy = torch.randn(S, N, device=DEV).half()
        dx = torch.full((S, K), -777.0, dtype=torch.float16, device=DEV)   # poison: rows past offsets[E] stay as they are
        assert lib.eetq_w8a16_moe_gemm_t(_ptr(dy), _ptr(w), _ptr(s), _ptr(offsets), _ptr(active), _ptr(dx), T, k, E, N, K,
                                         _stream()) == 0
        for e in range(E):
            if off[e + 1] == off[e]:
                continue
            rows = slice(off[e], off[e + 1])
            assert torch.equal(dx[rows], w8_a16_gemm_t(dy[rows], w[e], s[e])), (e, K, N)
        assert bool((dx[used:] == -777.0).all())
    if kind == "one" and T == 2048:
        assert int(counts.max()) > 128   # an expert with several row tiles
    if kind == "few":
        assert int((counts == 0).sum()) > 0


# ---- 2. gated-activation backward ---------------------------------------------------------------------------------------------
def _glu8_pack(g, u):
    """[rows, I] gate and up -> [rows, 2I] in glu8 order (8 gate + the matching 8 up per 16 columns)"""
    r, i = g.shape
    return torch.stack([g.reshape(r, i // 8, 8), u.reshape(r, i // 8, 8)], 2).reshape(r, 2 * i).contiguous()


def _glu8_unpack(gu):
    r, n = gu.shape
    v = gu.reshape(r, n // 16, 2, 8)
    return v[:, :, 0].reshape(r, n // 2), v[:, :, 1].reshape(r, n // 2)


@pytest.mark.parametrize("scale", [1.0, 4.0, 40.0, 3000.0])
def test_silu_mul_glu8_backward(lib, scale):
    rows, I = 37, 192
    torch.manual_seed(int(scale))
    g = (torch.randn(rows, I, device=DEV) * scale).half()
    u = torch.randn(rows, I, device=DEV).half()
    dh = torch.randn(rows, I, device=DEV).half()
    gu = _glu8_pack(g, u)
    dgu = torch.empty_like(gu)
    assert lib.eetq_silu_mul_glu8_bwd_f16(_ptr(gu), _ptr(dh), _ptr(dgu), rows, I, _stream()) == 0
    dg, du = _glu8_unpack(dgu)
    # du: torch's gradient of the forward's fp16 multiply silu(g) * u, bit for bit
    gg, uu = g.clone().requires_grad_(), u.clone().requires_grad_()
    (torch.nn.functional.silu(gg.float()).half() * uu).backward(dh)
    assert torch.equal(du, uu.grad)
    # dg: within 2 fp16 ulp of the fp32 formula
    g32, sig = g.float(), torch.sigmoid(g.float())
    ref = (dh.float() * u.float() * sig * (1 + g32 * (1 - sig))).cpu().numpy()
    ulp = np.spacing(np.abs(ref).astype(np.float16)).astype(np.float32)
    err = np.abs(dg.float().cpu().numpy() - ref)
    assert (err <= 2 * ulp).all(), float((err / ulp).max())


# ---- 3. combine backward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind", ["uniform", "sentinel", "dup"])
def test_combine_backward(lib, wdtype, kind):
    T, k, E, H = 37, 4, 16, 256
    idx = _routing(T, k, E, kind, seed=3)
    _, offsets, _, position, _ = _route(lib, idx, E)
    S = T * k
    y = torch.randn(S, H, device=DEV).half()
    dout = torch.randn(T, H, device=DEV).half()
    wts = _router_weights(T, k, seed=4).to(wdtype)
    dy = torch.full((S, H), -777.0, dtype=torch.float16, device=DEV)
    dw = torch.full((T, k), 5.0, dtype=wdtype, device=DEV)
    wd = 1 if wdtype == torch.float32 else 0
    assert lib.eetq_moe_combine_bwd_f16(_ptr(dout), _ptr(y), _ptr(position), _ptr(wts), wd, _ptr(dy), _ptr(dw), T, k, H,
                                        _stream()) == 0
    pos = position.view(T, k).long()
    live = pos >= 0
    for t in range(T):
        for j in range(k):
            p = int(pos[t, j])
            if p < 0:
                continue
            assert torch.equal(dy[p], (dout[t].float() * wts[t, j].float()).half()), (t, j)
    # dw against fp64; slots outside [0, E) get exactly 0
    prod = dout.double()[:, None, :] * y.double()[pos.clamp(min=0)]
    ref = prod.sum(-1)
    bound = 1e-4 * prod.abs().sum(-1)
    assert dw.dtype == wdtype
    assert bool(((dw.double() - ref).abs() <= bound)[live].all())
    assert bool((dw[~live] == 0).all()) and (kind != "sentinel" or bool((~live).any()))
    # dw = NULL: the same dy, no router gradient
    dy2 = torch.full_like(dy, -777.0)
    assert lib.eetq_moe_combine_bwd_f16(_ptr(dout), _ptr(y), _ptr(position), _ptr(wts), wd, _ptr(dy2), None, T, k, H,
                                        _stream()) == 0
    assert torch.equal(dy2, dy)


# ---- 4. layer gradients against float32 autograd on the dequantised stacks --------------------------------------------------
def _layer_ref(x, idx, wts, deq, E, act=torch.nn.functional.silu):
    """test_gpu_moe._layer_ref with a choice of activation (its autograd graph gives the float32 gradients)"""
    gu, dn = (d.float() for d in deq)
    I = dn.shape[1]
    T, k = idx.shape
    out = torch.zeros(x.shape, dtype=torch.float32, device=DEV)
    ids = idx.flatten()
    keep = ((ids >= 0) & (ids < E)).nonzero().flatten()
    e, tok = ids[keep], keep // k
    h = torch.bmm(x.float()[tok].unsqueeze(1), gu[e]).squeeze(1)
    a = act(h[:, :I]) * h[:, I:]
    d = torch.bmm(a.unsqueeze(1), dn[e]).squeeze(1) * wts.flatten().float()[keep, None]
    for j in range(k):
        sel = keep % k == j
        out = out.index_add(0, tok[sel], d[sel])
    return out


def _ref_grads(x, idx, wts, deq, E, G, act=torch.nn.functional.silu):
    xr = x.detach().float().requires_grad_()
    wr = wts.detach().float().requires_grad_()
    (_layer_ref(xr, idx, wr, deq, E, act) * G).sum().backward()
    return xr.grad, wr.grad


def _silu_without_its_derivative_term(a):
    return a * torch.sigmoid(a).detach()   # d/da = sigma: the dg = dh * u * sigma mistake


@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 64, 8)])
@pytest.mark.parametrize("T", [1, 2, 3, 7, 16, 17, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_layer_gradients_against_fp32_reference(lib, E, H, I, k, T, kind):
    _, q, deq = _experts(E, H, I, k, seed=E + H)
    q.trainable = True
    x = torch.randn(T, H, device=DEV).half().requires_grad_()
    idx = _routing(T, k, E, kind, seed=T)
    wts = _router_weights(T, k, seed=T + 1).requires_grad_()
    G = torch.randn(T, H, device=DEV)
    (q(x, idx, wts).float() * G).sum().backward()
    assert x.grad.dtype == torch.float16 and wts.grad.dtype == torch.float32
    gx, gw = _ref_grads(x, idx, wts, deq, E, G)
    assert gx.abs().max() > 0.1
    assert _close(x.grad, gx), (x.grad.float() - gx).abs().max().item()
    assert _close(wts.grad, gw), (wts.grad.float() - gw).abs().max().item()
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


# ---- 5. trainable forward == inference forward; who gets a grad_fn ---------------------------------------------------------
@pytest.mark.parametrize("T", [1, 16, 17, 100])
@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 64, 8)])
def test_trainable_forward_is_the_inference_forward(E, H, I, k, T):
    _, q, _ = _experts(E, H, I, k, seed=11)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "sentinel", seed=T)
    wts = _router_weights(T, k, seed=T)
    with torch.no_grad():
        want = q(x, idx, wts)
    xg, wg = x.clone().requires_grad_(), wts.clone().requires_grad_()
    assert q(xg, idx, wg).grad_fn is None                      # default: inference only, as before
    q.trainable = True
    got = q(xg, idx, wg)
    assert got.grad_fn is not None and torch.equal(got, want)
    assert torch.equal(q(x, idx, wg), want) and q(x, idx, wg).grad_fn is not None
    assert q(x, idx, wts).grad_fn is None                      # nothing requires grad
    with torch.no_grad():
        assert q(xg, idx, wg).grad_fn is None


def test_trainable_linear():
    from eetq_amd.modules.qlinear import W8A16Linear
    torch.manual_seed(0)
    lin = torch.nn.Linear(256, 384, bias=True).half().to(DEV)
    q = W8A16Linear.from_torch(lin)
    x = torch.randn(5, 256, device=DEV).half().requires_grad_()
    with torch.no_grad():
        want = q(x)
    assert q(x).grad_fn is None
    q.trainable = True
    y = q(x)
    assert y.grad_fn is not None and torch.equal(y, want)
    y.float().sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape
    assert q(x, residual=torch.zeros(5, 384, dtype=torch.float16, device=DEV)).grad_fn is None   # extensions stay inference-only


# ---- 6. no host sync (graph capture) and determinism --------------------------------------------------------------------------
def test_backward_is_capturable_and_deterministic():
    from eetq_amd.ops import w8_a16_moe_backward, w8_a16_moe_train
    _, q, _ = _experts(8, 256, 128, 2, seed=2)
    T, k, E = 64, 2, 8
    x = torch.randn(T, 256, device=DEV).half()
    idx = _routing(T, k, E, "sentinel", seed=5)
    wts = _router_weights(T, k, seed=6)
    stacks = (q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)
    out, tables, gate_up, y = w8_a16_moe_train(x, idx, wts, *stacks)
    dout = torch.randn(T, 256, device=DEV).half()
    a = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
    b = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gx, gw = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
    for seed in (1, 2):
        dout.copy_(torch.randn(T, 256, generator=torch.Generator().manual_seed(seed)).half())
        g.replay()
        torch.cuda.synchronize()
        fx, fw = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
        assert torch.equal(gx, fx) and torch.equal(gw, fw)
    # only what is asked for
    nx, nw = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, False, True)
    assert nx is None and torch.equal(nw, fw)
    nx, nw = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, False)
    assert nw is None and torch.equal(nx, fx)


# ---- 7. memory ----------------------------------------------------------------------------------------------------------------
def test_backward_memory_is_activations_only():
    from eetq_amd.ops import w8_a16_moe_backward, w8_a16_moe_train
    E, H, I, k, T = 8, 4096, 14336, 2, 512
    gu_w, gu_s = _random_stack(E, H, 2 * I)
    dn_w, dn_s = _random_stack(E, I, H)
    x = (torch.rand(T, H, device=DEV) - 0.5).half()
    idx = _routing(T, k, E, "uniform", seed=1)
    wts = _router_weights(T, k, seed=2)
    _, tables, gate_up, y = w8_a16_moe_train(x, idx, wts, gu_w, gu_s, dn_w, dn_s)
    dout = torch.randn(T, H, device=DEV).half()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    gx, gw = w8_a16_moe_backward(dout, wts, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s, True, True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    S = T * k
    bound = 2 * S * (3 * I + H) + 2 * T * H + (1 << 20)
    assert peak <= bound, (peak, bound)
    assert peak < E * H * 2 * I * 2 / 10                  # a tenth of one dequantised fp16 gate|up stack
    assert torch.isfinite(gx.float()).all() and torch.isfinite(gw).all()


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------
def _dequantised_fp32_copy(model):
    """float32 copy of an fp16 model whose projections and expert stacks hold fp16(q s) of their int8 quantisation"""
    from eetq_amd.ops import quant_weights
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for name, m in ref.named_modules():
            if isinstance(m, torch.nn.Linear) and "lm_head" not in name:
                raw, _, s = quant_weights(m.weight.t().contiguous(), torch.int8, True)
                m.weight.copy_((raw.float() * s.float()[None, :]).half().t())
        for layer in ref.model.layers:
            ex = layer.mlp.experts
            for p in (ex.gate_up_proj, ex.down_proj):
                raw, _, s = quant_weights(p.transpose(1, 2).contiguous(), torch.int8, True)
                p.copy_((raw.float() * s.float()[:, None, :]).half().transpose(1, 2))
    return ref.float()


def _grads(model, emb, G):
    model.zero_grad(set_to_none=True)
    e = emb.detach().clone().requires_grad_()
    (model(inputs_embeds=e).logits.float() * G).sum().backward()
    routers = [layer.mlp.gate.weight.grad for layer in model.model.layers]
    return e.grad, routers


def _bound(got, ref):
    if got is None:
        return False
    got, ref = got.float(), ref.float()
    return bool(((got - ref).abs() <= 2e-2 * ref.abs().max() + 2e-2 * ref.abs()).all())


@pytest.mark.parametrize("which", ["mixtral", "qwen3_moe"])
def test_end_to_end_gradients(which):
    from eetq_amd.utils import eet_quantize, set_trainable
    model = _tiny(which)
    ref = _dequantised_fp32_copy(model)
    eet_quantize(model, experts=True, trainable=True)
    ids = torch.randint(0, 512, (2, 12), generator=torch.Generator().manual_seed(3)).to(DEV)
    emb = model.model.embed_tokens(ids).detach()
    G = torch.randn(2, 12, 512, generator=torch.Generator().manual_seed(4)).to(DEV)
    ref_x, ref_r = _grads(ref, emb.float(), G)
    got_x, got_r = _grads(model, emb, G)
    assert _bound(got_x, ref_x), (got_x.float() - ref_x).abs().max().item() / ref_x.abs().max().item()
    for g, r in zip(got_r, ref_r):
        assert r.abs().max() > 0 and _bound(g, r), (g.float() - r).abs().max().item() / r.abs().max().item()
    # today's default (no opt-in): the experts and projections are cut out of the graph and the bound fails
    set_trainable(model, False)
    off_x, off_r = _grads(model, emb, G)
    assert not (_bound(off_x, ref_x) and all(_bound(g, r) for g, r in zip(off_r, ref_r)))
    set_trainable(model, True)
    # one decoder layer under non-reentrant checkpointing: the same gradients, bit for bit (eager attention: its backward has
    # no atomics)
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
