"""The MoE router on the device: logits against a float64 reference, the selection exactly (against the kernel's own
logits) and against the truth, the scores, the route tables against eetq_moe_route, the fused launch against the selection kernel,
the block ops against the layer ops bit for bit, repeat launches, graph replay, and tiny models after eet_quantize(router=True).

Bounds (none derived from what the kernels return):
  logits  |d| <= tau = 2^-11 |ref| + gamma, gamma = H 2^-24 sum_h |x_h w_eh|: half an fp16 ulp (one rounding of the exact sum)
          plus the worst-case error of an fp32 summation of H exact products in any order; inputs scaled to max|logit| = 5;
  scores  fp32 within 2^-18 relative of the float64 softmax / renormalisation of the kernel's own fp16 logits at its own indices
          (exp argument reduction at |x| <= 16, a few ulps of the sum, the division); fp16 within one fp16 ulp more; renormalised
          fp32 rows sum to 1 within k 2^-23."""
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(8, 4096, 2), (128, 2048, 8), (64, 2048, 8), (60, 2048, 4), (256, 512, 16)]
TOKENS = [1, 2, 4, 16, 17, 64, 512]
F16, F32 = 0, 1


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


def _inputs(T, E, H, seed):
    """fp16 x [T, H], w [E, H] with max|logit| = 5 (w rescaled from the float64 logits, then rounded to fp16)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, H)).astype(np.float16)
    w = (rng.standard_normal((E, H)) / np.sqrt(H)).astype(np.float16)
    w = (w.astype(np.float64) * (5.0 / np.abs(x.astype(np.float64) @ w.astype(np.float64).T).max())).astype(np.float16)
    return x, w


def _teeth(ref, tau, k):
    """fraction of tokens for which swapping the (k+3)-th best expert (by the float64 logits) in fails the truth check"""
    order = np.argsort(-ref, axis=1, kind="stable")
    kth, bad = order[:, k - 1:k], order[:, k + 2:k + 3]
    slack = np.take_along_axis(tau, bad, axis=1) + np.take_along_axis(tau, kth, axis=1)
    return (np.take_along_axis(ref, bad, axis=1) < np.take_along_axis(ref, kth, axis=1) - slack).mean()


def _inputs_with_teeth(T, E, H, k, seed):
    """_inputs at the first of seeds seed, seed + 1, ... (chosen on the CPU, from the reference alone) for which the truth check has
    teeth: the (k+3)-th expert swapped in fails it for most tokens"""
    for s in range(seed, seed + 20):
        x, w = _inputs(T, E, H, s)
        ref, tau = _ref(x, w)
        if _teeth(ref, tau, k) > 0.5:
            return x, w, ref, tau
    pytest.fail("no seed in %d..%d separates the (k+3)-th expert from the k-th for most tokens" % (seed, seed + 19))


def _ref(x, w):
    """float64 logits of the fp16 inputs and the bound tau on an fp16 logit computed with fp32 accumulation"""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref = x64 @ w64.T
    gamma = x.shape[1] * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T)
    return ref, 2.0 ** -11 * np.abs(ref) + gamma


def _scores64(logits16, idx, renorm):
    l = logits16.astype(np.float64)
    p = np.exp(l - l.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    s = np.take_along_axis(p, idx, axis=1)
    return s / s.sum(axis=1, keepdims=True) if renorm else s


def _ulp16(v):
    return 2.0 ** np.maximum(np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -24))) - 10, -24)


def _stable_topk(logits16, k):
    return np.argsort(-logits16.astype(np.float32), axis=1, kind="stable")[:, :k]


def _check_scores(scores, logits16, idx, renorm, k):
    want = _scores64(logits16, idx, renorm)
    got = scores.astype(np.float64)
    if scores.dtype == np.float32:
        rel = np.abs(got - want) / want
        print("fp32 scores: max relative error %.3g (bound %.3g)" % (rel.max(), 2.0 ** -18))
        assert rel.max() <= 2.0 ** -18
        if renorm:
            assert np.abs(got.sum(axis=1) - 1.0).max() <= k * 2.0 ** -23
    else:
        err = np.abs(got - want) - 2.0 ** -18 * want
        assert (err <= _ulp16(want)).all()


def _c_router(lib, x, w, k, renorm, dt, tables=True):
    """eetq_moe_router_f16 on device tensors -> (logits, idx, scores, [counts, offsets, sorted, position, active] or None)"""
    T, H = x.shape
    E = w.shape[0]
    S, A = T * k, min(E, T * k)
    logits = torch.full((T, E), -777.0, dtype=torch.float16, device=DEV)
    idx = torch.full((T, k), -5, dtype=torch.int64, device=DEV)
    sc = torch.full((T, k), -777.0, dtype=torch.float32 if dt == F32 else torch.float16, device=DEV)
    tb = [torch.full((n,), -9, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)] if tables else None
    tp = [_ptr(t) for t in tb] if tables else [None] * 5
    st = lib.eetq_moe_router_f16(_ptr(x), _ptr(w), T, H, E, k, renorm, dt, _ptr(logits), _ptr(idx), _ptr(sc), *tp, _stream())
    assert st == 0, lib.eetq_last_error()
    return logits, idx, sc, tb


def _c_route(lib, idx, E):
    T, k = idx.shape
    S, A = T * k, min(E, T * k)
    tb = [torch.full((n,), -9, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)]
    assert lib.eetq_moe_route(_ptr(idx), T, k, E, *[_ptr(t) for t in tb], _stream()) == 0, lib.eetq_last_error()
    return tb


@pytest.mark.parametrize("E,H,k", SHAPES)
@pytest.mark.parametrize("T", TOKENS)
def test_router_entry_logits_selection_scores_tables(lib, E, H, k, T):
    """the C entry at every shape and T (the fused launch at T <= 16, the chunked kernels above), both score dtypes, both renorm"""
    x, w, ref, tau = _inputs_with_teeth(T, E, H, k, seed=1000 + T + E)
    assert 2.0 <= np.abs(ref).max() <= 8.0
    assert _teeth(ref, tau, k) > 0.5      # on this very data the (k+3)-th expert swapped in fails the truth check below
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    first = None
    for dt in (F32, F16):
        for renorm in (1, 0):
            logits, idx, sc, tb = _c_router(lib, xd, wd, k, renorm, dt)
            torch.cuda.synchronize()
            l16, ix, s = logits.cpu().numpy(), idx.cpu().numpy(), sc.cpu().numpy()
            if first is None:
                err = np.abs(l16.astype(np.float64) - ref)
                print("logits: max |err| / tau = %.3f" % (err / tau).max())
                assert (err <= tau).all()
                # the bound has teeth: nothing, and the neighbouring expert's logit, both fail it
                assert not (np.abs(0.0 - ref) <= tau).all()
                assert not (np.abs(np.roll(l16.astype(np.float64), 1, axis=1) - ref) <= tau).all()
                first = (l16, ix)
            else:  # the logits and the selection depend on neither flag
                assert np.array_equal(l16, first[0]) and np.array_equal(ix, first[1])
            assert np.array_equal(ix, _stable_topk(l16, k))
            # against the truth: no selected expert is worse than the k-th best by more than the two logits' bounds
            order = np.argsort(-ref, axis=1, kind="stable")
            kth = order[:, k - 1:k]
            slack = np.take_along_axis(tau, ix, axis=1) + np.take_along_axis(tau, kth, axis=1)
            assert (np.take_along_axis(ref, ix, axis=1) >= np.take_along_axis(ref, kth, axis=1) - slack).all()
            _check_scores(s, l16, ix, renorm, k)
            want = _c_route(lib, idx, E)
            torch.cuda.synchronize()
            for name, a, b in zip(("counts", "offsets", "sorted_slot", "position", "active"), tb, want):
                assert torch.equal(a, b), name
    # no tables: the same outputs
    logits, idx, sc, _ = _c_router(lib, xd, wd, k, 0, F16, tables=False)
    assert np.array_equal(logits.cpu().numpy(), first[0]) and np.array_equal(idx.cpu().numpy(), first[1])


@pytest.mark.parametrize("E,H,k", SHAPES)
@pytest.mark.parametrize("T", TOKENS)
def test_ops_moe_router(E, H, k, T):
    """ops.moe_router (at::linear logits above T = 16): the same contract through the extension"""
    from eetq_amd.ops import moe_router
    x, w = _inputs(T, E, H, seed=2000 + T + E)
    ref, tau = _ref(x, w)
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    for dtype in (torch.float32, torch.float16):
        for renorm in (True, False):
            logits, scores, idx = moe_router(xd, wd, k, renorm, dtype)
            assert logits.dtype == torch.float16 and scores.dtype == dtype and idx.dtype == torch.int64
            assert logits.shape == (T, E) and scores.shape == (T, k) and idx.shape == (T, k)
            l16, ix = logits.cpu().numpy(), idx.cpu().numpy()
            assert (np.abs(l16.astype(np.float64) - ref) <= tau).all()
            assert np.array_equal(ix, _stable_topk(l16, k))
            _check_scores(scores.cpu().numpy(), l16, ix, renorm, k)
    logits, scores, idx = moe_router(xd[:0], wd, k)
    assert logits.shape == (0, E) and scores.shape == (0, k) and scores.dtype == torch.float32 and idx.shape == (0, k)


@pytest.mark.parametrize("T", [3, 16, 40])
def test_exact_ties(lib, T):
    """duplicated router rows give equal logits: the lower id wins; all rows equal: experts 0 .. k-1 with equal scores"""
    E, H, k = 64, 2048, 8
    x, w = _inputs(T, E, H, seed=7)
    w[1::2] = w[0::2]  # every odd row repeats the even row before it
    xd = torch.from_numpy(x).to(DEV)
    logits, idx, sc, _ = _c_router(lib, xd, torch.from_numpy(w).to(DEV), k, 1, F32)
    l16, ix = logits.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(l16[:, 0::2], l16[:, 1::2])
    assert np.array_equal(ix, _stable_topk(l16, k))
    assert (ix[:, 0::2] % 2 == 0).all() and np.array_equal(ix[:, 1::2], ix[:, 0::2] + 1)
    w[:] = w[0]
    for renorm in (1, 0):
        logits, idx, sc, _ = _c_router(lib, xd, torch.from_numpy(w).to(DEV), k, renorm, F32)
        l16 = logits.cpu().numpy()
        assert (l16 == l16[:, :1]).all()
        assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(k), (T, 1)))
        np.testing.assert_allclose(sc.cpu().numpy(), 1.0 / (k if renorm else E), rtol=2.0 ** -18)


@pytest.mark.parametrize("E,H,k", SHAPES)
@pytest.mark.parametrize("T", [1, 4, 16])
def test_fused_launch_and_selection_kernel_give_the_same_bits(lib, E, H, k, T):
    x, w = _inputs(T, E, H, seed=31 + T)
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    for dt in (F32, F16):
        for renorm in (1, 0):
            logits, idx, sc, _ = _c_router(lib, xd, wd, k, renorm, dt)
            idx2, sc2 = torch.full_like(idx, -5), torch.full_like(sc, -777.0)
            assert lib.eetq_moe_topk_f16(_ptr(logits), T, E, k, renorm, dt, _ptr(idx2), _ptr(sc2), _stream()) == 0
            assert torch.equal(idx, idx2) and torch.equal(sc.view(torch.uint8), sc2.view(torch.uint8))


def _experts(E, H, I, k, bits, seed):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd.modules.qlinear import W4A16Experts, W8A16Experts
    torch.manual_seed(seed)
    src = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)).half().to(DEV)
    with torch.no_grad():
        src.gate_up_proj.normal_(0, 1.5 / H ** 0.5)
        src.down_proj.normal_(0, 2.0 / I ** 0.5)
    q = (W4A16Experts if bits == 4 else W8A16Experts).from_experts(src)
    return q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales


@pytest.mark.parametrize("E,H,k", SHAPES)
@pytest.mark.parametrize("bits", [8, 4])
def test_block_ops_equal_the_layer_ops_on_the_routers_output(E, H, k, bits):
    from eetq_amd import ops
    I = 384
    stacks = _experts(E, H, I, k, bits, seed=5)
    for T in TOKENS:
        x, w = _inputs(T, E, H, seed=3000 + T)
        xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
        for dtype, renorm in ((torch.float32, True), (torch.float16, False)):
            routed = ops.moe_router(xd, wd, k, renorm, dtype)
            if bits == 8:
                want = ops.w8_a16_moe(xd, *routed[2:0:-1], *stacks)
                got = ops.w8_a16_moe_block(xd, wd, k, renorm, dtype, *stacks)
                assert torch.equal(got, want), (T, dtype)
                continue
            for path in ("auto", "decode", "expand"):   # expand at T <= 16 too: the fused front feeding the expanded stacks
                want = ops.w4_a16_moe(xd, *routed[2:0:-1], *stacks, path=path)
                got = ops.w4_a16_moe_block(xd, wd, k, renorm, dtype, *stacks, path=path)
                assert torch.equal(got, want), (T, dtype, path)
            assert torch.isfinite(got).all() and got.abs().max() > 0


@pytest.mark.parametrize("E,H,k", [(8, 4096, 2), (128, 2048, 8)])
def test_fifty_back_to_back_launches_give_the_same_bits(E, H, k):
    """guards the hand-over: every launch's finishing workgroup must see every other workgroup's sums"""
    from eetq_amd.ops import moe_router
    x, w = _inputs(4, E, H, seed=11)
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    runs = [moe_router(xd, wd, k, True, torch.float32) for _ in range(50)]
    torch.cuda.synchronize()
    ref, tau = _ref(x, w)
    assert (np.abs(runs[0][0].cpu().numpy().astype(np.float64) - ref) <= tau).all()
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("T", [4, 64])
@pytest.mark.parametrize("bits", [8, 4])
def test_block_op_graph_replay(T, bits):
    from eetq_amd import ops
    E, H, k, I = 64, 2048, 8, 384
    stacks = _experts(E, H, I, k, bits, seed=9)
    op = ops.w8_a16_moe_block if bits == 8 else ops.w4_a16_moe_block
    x, w = _inputs(T, E, H, seed=77)
    x2, _ = _inputs(T, E, H, seed=78)
    hidden, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    op(hidden, wd, k, True, torch.float16, *stacks)  # warm-up: the hand-over slot is created outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = op(hidden, wd, k, True, torch.float16, *stacks)
    hidden.copy_(torch.from_numpy(x2))
    g.replay()
    torch.cuda.synchronize()
    fresh = op(torch.from_numpy(x2).to(DEV), wd, k, True, torch.float16, *stacks)
    assert torch.equal(out, fresh)
    assert not torch.equal(fresh, op(torch.from_numpy(x).to(DEV), wd, k, True, torch.float16, *stacks))


def _tiny(kind):
    import transformers as tf
    common = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, vocab_size=256)
    if kind == "mixtral":
        cfg = tf.MixtralConfig(intermediate_size=256, num_key_value_heads=2, num_local_experts=8, num_experts_per_tok=2, **common)
        return tf.MixtralForCausalLM(cfg)
    if kind == "qwen3":
        cfg = tf.Qwen3MoeConfig(intermediate_size=256, moe_intermediate_size=128, num_key_value_heads=2, num_experts=16,
                                num_experts_per_tok=4, decoder_sparse_step=1, mlp_only_layers=[], **common)
        return tf.Qwen3MoeForCausalLM(cfg)
    cfg = tf.OlmoeConfig(intermediate_size=128, num_key_value_heads=4, num_experts=16, num_experts_per_tok=4, **common)
    return tf.OlmoeForCausalLM(cfg)


@pytest.mark.parametrize("kind", ["mixtral", "qwen3", "olmoe"])
def test_models_with_and_without_the_device_router(kind):
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter
    from eetq_amd.utils.quantizer import eet_quantize
    torch.manual_seed(3)
    base = _tiny(kind).half().to(DEV).eval()
    with torch.no_grad():
        for layer in base.model.layers:
            layer.mlp.gate.weight.normal_(0, 0.5)
    plain, routed = copy.deepcopy(base), copy.deepcopy(base)
    eet_quantize(plain, experts=True)
    eet_quantize(routed, experts=True, router=True)
    assert all(isinstance(l.mlp, EetqSparseMoeBlock) and isinstance(l.mlp.gate, EetqTopKRouter) for l in routed.model.layers)
    assert not any(isinstance(m, (EetqSparseMoeBlock, EetqTopKRouter)) for m in plain.modules())
    ids = torch.randint(0, 256, (2, 7), device=DEV)
    seen = {}

    def hook(tag):
        return lambda mod, args, out: seen.__setitem__(tag, (args[0].detach().reshape(-1, 128).cpu().numpy(), out[0].cpu().numpy()))
    h1 = plain.model.layers[0].mlp.gate.register_forward_hook(hook("plain"))
    h2 = routed.model.layers[0].mlp.gate.register_forward_hook(hook("routed"))
    with torch.no_grad():
        a = plain(ids).logits
        b = routed(ids).logits      # layer 0 is observed (unfused, device router); layer 1 runs the block op
    h1.remove()
    h2.remove()
    assert np.array_equal(seen["plain"][0], seen["routed"][0])           # layer 0's MoE input is the same in both
    ref, tau = _ref(seen["plain"][0], routed.model.layers[0].mlp.gate.weight.detach().cpu().numpy())
    for tag in ("plain", "routed"):
        assert (np.abs(seen[tag][1].astype(np.float64) - ref) <= tau).all(), tag
    with torch.no_grad():
        c = routed(ids).logits      # no hooks: both layers run the block op
        d = routed(ids).logits
        one = routed(ids[:1, :1]).logits
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.isfinite(c).all() and torch.isfinite(one).all()
    assert torch.equal(c, d)
    assert torch.equal(b, c)        # the block op is the bits of gate -> experts
    # a call that needs gradients reaches the original forward: the unswapped router's gradients
    gate, ref_gate = routed.model.layers[0].mlp.gate, base.model.layers[0].mlp.gate
    grads = []
    for g in (gate, ref_gate):
        x = torch.randn(5, 128, device=DEV, dtype=torch.float16, generator=torch.Generator(DEV).manual_seed(1)).requires_grad_(True)
        g.weight.grad = None
        logits, scores, idx = g(x)
        (scores.float().sum() + logits.float().pow(2).sum()).backward()
        grads.append((x.grad.clone(), g.weight.grad.clone(), idx))
    assert all(torch.equal(p, q) for p, q in zip(*grads))
    assert grads[0][0].abs().max() > 0


def test_output_router_logits_keeps_working():
    """transformers records router logits with forward hooks on the gates, installed the first time any output_* flag is asked for:
    from then on the blocks call their gate (unfused path, device router) and the logits come back, one [T, E] per layer"""
    from eetq_amd.utils.quantizer import eet_quantize
    torch.manual_seed(3)
    base = _tiny("mixtral").half().to(DEV).eval()
    plain, routed = copy.deepcopy(base), copy.deepcopy(base)
    eet_quantize(plain, experts=True)
    eet_quantize(routed, experts=True, router=True)
    ids = torch.randint(0, 256, (2, 7), device=DEV)
    with torch.no_grad():
        assert all(layer.mlp.fused(torch.zeros(1, 1, 128, device=DEV, dtype=torch.float16)) for layer in routed.model.layers)
        before = routed(ids).logits
        want = plain(ids, output_router_logits=True)
        got = routed(ids, output_router_logits=True)
        assert not any(layer.mlp.fused(torch.zeros(1, 1, 128, device=DEV, dtype=torch.float16)) for layer in routed.model.layers)
        after = routed(ids).logits
    assert got.router_logits is not None and len(got.router_logits) == len(want.router_logits) == 2
    seen = {}
    h = routed.model.layers[0].mlp.gate.register_forward_hook(
        lambda m, a, o: seen.__setitem__("x", a[0].detach().reshape(-1, 128).cpu().numpy()))
    with torch.no_grad():
        routed(ids)
    h.remove()
    ref, tau = _ref(seen["x"], routed.model.layers[0].mlp.gate.weight.detach().cpu().numpy())
    for out in (got, want):
        l0 = out.router_logits[0]
        assert l0.shape == (14, 8) and l0.dtype == torch.float16
        assert (np.abs(l0.cpu().numpy().astype(np.float64) - ref) <= tau).all()
    assert torch.equal(got.logits, before) and torch.equal(after, before)   # fused or not: the same bits
