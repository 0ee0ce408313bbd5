"""The sigmoid, bias-corrected, group-limited MoE router on the device.  The checks chain, and no bound is taken
from what the kernels return:
  1. logits   |fp32 logit - float64 reference| <= gamma = H 2^-24 sum_h |x_h w_eh| (an fp32 summation in any order; no fp16 rounding);
  2. selection against the float64 restatement (test_moe_router_sigmoid_cpu.restate) run on the kernel's OWN fp32 logits.
              delta = 2^-21 bounds the kernel's error in c.  A token is separated when the restated group margin is above 8 delta and
              the restated margin between the k-th and (k+1)-th expert above 2 delta: there the index set is the restatement's, in
              descending order of c (up to the 2 delta by which two fp32 c may swap); on every token each selected expert lies in a
              group whose restated score is within 4 delta of the KG-th best.  At least 95 % of a case's tokens must be separated;
  3. the truth: on tokens (chosen on the CPU, from the reference alone) that are separated at the logit level -- group margin
              > 4 eps, expert margin > 2 eps, eps = 0.25 max gamma + delta (|d sigmoid / d logit| <= 0.25) -- the index set is the
              float64 reference's own;
  4. weights  fp32 within 2^-18 relative of the float64 formula on the kernel's own logits and indices; fp16 one fp16 ulp more;
  5. tables   equal to eetq_moe_route on the emitted indices;
  6. ties, 7. the fused launch against the selection kernel, 8. the block ops against router op + layer op, 9. determinism, graph
  replay and interleaving with the softmax router, 10. tiny DeepSeek-V3 and GLM-4-MoE models."""
import copy
import functools

import numpy as np
import pytest
import torch

from test_gpu_moe_router import _c_route, _experts, _ptr, _stream, _ulp16
from test_gpu_moe_router import _inputs as _softmax_inputs
from test_moe_router_sigmoid_cpu import DELTA, SHAPES, inputs, ref_logits, restate, separated, tiny, weights64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOKENS = [1, 4, 16, 17, 64]
F16, F32 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    L = _lib.lib()
    assert L.eetq_device_supported() == 1, "kernels are built for gfx950 only"
    return L


@functools.lru_cache(maxsize=None)
def _case(T, E, H, seed):
    """inputs, float64 logits and gamma, computed once per case and left unchanged"""
    x, w, bias = inputs(T, E, H, seed)
    ref, gamma = ref_logits(x, w)
    for a in (x, w, bias, ref, gamma):
        a.setflags(write=False)
    return x, w, bias, ref, gamma


def _dev(a):
    return torch.tensor(a, device=DEV)   # a copy: the cached cases are read-only


def _c_router(lib, x, w, bias, k, G, KG, renorm, scale, dt, tables=True):
    """eetq_moe_router_sigmoid_f16 on device tensors -> (logits fp32, idx, weights, [counts, offsets, sorted, position, active])"""
    T, H = x.shape
    E = w.shape[0]
    S, A = T * k, min(E, T * k)
    logits = torch.full((T, E), -777.0, dtype=torch.float32, device=DEV)
    idx = torch.full((T, k), -5, dtype=torch.int64, device=DEV)
    wts = torch.full((T, k), -777.0, dtype=torch.float32 if dt == F32 else torch.float16, device=DEV)
    tb = [torch.full((n,), -9, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)] if tables else None
    tp = [_ptr(t) for t in tb] if tables else [None] * 5
    bdt = F32 if bias.dtype == torch.float32 else F16
    st = lib.eetq_moe_router_sigmoid_f16(_ptr(x), _ptr(w), _ptr(bias), bdt, T, H, E, k, G, KG, renorm, scale, dt, _ptr(logits), _ptr(idx),
                                         _ptr(wts), *tp, _stream())
    assert st == 0, lib.eetq_last_error()
    return logits, idx, wts, tb


def _c_topk(lib, logits, bias, k, G, KG, renorm, scale, dt):
    T, E = logits.shape
    idx = torch.full((T, k), -5, dtype=torch.int64, device=DEV)
    wts = torch.full((T, k), -777.0, dtype=torch.float32 if dt == F32 else torch.float16, device=DEV)
    bdt = F32 if bias.dtype == torch.float32 else F16
    st = lib.eetq_moe_topk_sigmoid_f32(_ptr(logits), _ptr(bias), bdt, T, E, k, G, KG, renorm, scale, dt, _ptr(idx), _ptr(wts), _stream())
    assert st == 0, lib.eetq_last_error()
    return idx, wts


def _check_logits(l32, ref, gamma):
    err = np.abs(l32.astype(np.float64) - ref)
    print("logits: max |err| / gamma = %.3f" % (err / gamma).max())
    assert (err <= gamma).all()
    # the bound has teeth: nothing, and the neighbouring expert's logit, both fail it
    assert not (np.abs(0.0 - ref) <= gamma).all()
    if ref.shape[1] > 1:
        assert not (np.abs(np.roll(l32.astype(np.float64), 1, axis=1) - ref) <= gamma).all()


def _check_selection(l32, bias, ix, k, G, KG):
    """check 2, on the kernel's own logits"""
    r = restate(l32, bias, k, G, KG)
    sep = separated(r, 8 * DELTA, 2 * DELTA)
    print("separated %d / %d; smallest margins: group %.3g, expert %.3g" % (sep.sum(), len(sep), r.gmargin.min(), r.emargin.min()))
    assert sep.mean() >= 0.95
    assert (np.sort(ix[sep], axis=1) == np.sort(r.idx[sep], axis=1)).all()
    assert all(len(set(row)) == k for row in ix.tolist())
    c_sel = np.take_along_axis(r.c, ix, axis=1)
    assert (c_sel[sep][:, :-1] >= c_sel[sep][:, 1:] - 2 * DELTA).all()
    per = l32.shape[1] // G
    g_sel = np.take_along_axis(r.gscore, ix // per, axis=1)
    assert (g_sel >= r.kth_gscore[:, None] - 4 * DELTA).all()
    return r


def _check_weights(wts, l32, ix, renorm, scale):
    want = weights64(l32, ix, renorm, scale)
    got = wts.astype(np.float64)
    if wts.dtype == np.float32:
        rel = np.abs(got - want) / want
        print("fp32 weights: max relative error %.3g (bound %.3g)" % (rel.max(), 2.0 ** -18))
        assert rel.max() <= 2.0 ** -18
    else:
        assert (np.abs(got - want) - 2.0 ** -18 * want <= _ulp16(want)).all()


@pytest.mark.parametrize("E,H,k,G,KG", SHAPES)
@pytest.mark.parametrize("T", TOKENS)
def test_entry_logits_selection_weights_tables(lib, E, H, k, G, KG, T):
    """checks 1, 2, 4 and 5 on the C entry: the fused launch at T <= 16, the chunked kernels above; both weight dtypes, both bias
    dtypes, with and without norm_topk_prob, scale 1 and 2.5"""
    x, w, bias, ref, gamma = _case(T, E, H, 1000 + T + E)
    assert 2.0 <= np.abs(ref).max() <= 8.0
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    first = None
    for dt, renorm, scale in ((F32, 1, 2.5), (F32, 0, 1.0), (F16, 1, 1.0), (F16, 0, 2.5)):
        logits, idx, wts, tb = _c_router(lib, xd, wd, bd, k, G, KG, renorm, scale, dt)
        torch.cuda.synchronize()
        l32, ix, wt = logits.cpu().numpy(), idx.cpu().numpy(), wts.cpu().numpy()
        if first is None:
            _check_logits(l32, ref, gamma)
            _check_selection(l32, bias, ix, k, G, KG)
            first = (l32, ix)
        else:  # the logits and the selection depend on none of the three
            assert np.array_equal(l32, first[0]) and np.array_equal(ix, first[1])
        _check_weights(wt, l32, ix, renorm, scale)
        want = _c_route(lib, idx, E)
        torch.cuda.synchronize()
        for name, a, b in zip(("counts", "offsets", "sorted_slot", "position", "active"), tb, want):
            assert torch.equal(a, b), name
    # no tables: the same outputs
    logits, idx, wts, _ = _c_router(lib, xd, wd, bd, k, G, KG, 0, 2.5, F16, tables=False)
    assert np.array_equal(logits.cpu().numpy(), first[0]) and np.array_equal(idx.cpu().numpy(), first[1])
    assert np.array_equal(wts.cpu().numpy(), wt)
    # an fp16 bias (the buffer after model.half()): the same contract on the rounded bias, no cast launched
    b16 = bias.astype(np.float16)
    logits, idx, wts, _ = _c_router(lib, xd, wd, _dev(b16), k, G, KG, 1, 2.5, F32)
    l32, ix = logits.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(l32, first[0])
    _check_selection(l32, b16, ix, k, G, KG)
    _check_weights(wts.cpu().numpy(), l32, ix, 1, 2.5)


@functools.lru_cache(maxsize=None)
def _logit_separated_tokens(E, H, k, G, KG):
    """The first 16 tokens of a pool of 256 (one seed: one weight, one bias) that are separated at the logit level, chosen from the
    float64 reference alone, with the reference's selection for them.  eps takes the pool's largest gamma.  Whole seeds cannot do this
    at H = 7168: there gamma is so large that one token in six is separated, so 16 random tokens are all separated once in 10^12
    seeds (T = 4: once in 10^3); the pool holds about 80 such tokens."""
    x, w, bias, ref, gamma = _case(256, E, H, 5000 + E)
    eps = 0.25 * gamma.max() + DELTA
    r = restate(ref, bias, k, G, KG)
    rows = np.flatnonzero(separated(r, 4 * eps, 2 * eps))[:16]
    assert len(rows) == 16, "fewer than 16 of 256 tokens are separated at the logit level"
    return x[rows], w, bias, r.idx[rows]


@pytest.mark.parametrize("E,H,k,G,KG", SHAPES[:3] + [(16, 128, 4, 4, 2)])
@pytest.mark.parametrize("T", [1, 4, 16])
def test_selection_against_the_truth(lib, E, H, k, G, KG, T):
    """check 3"""
    x, w, bias, truth = _logit_separated_tokens(E, H, k, G, KG)
    _, idx, _, _ = _c_router(lib, _dev(x[:T]), _dev(w), _dev(bias), k, G, KG, 1, 1.0, F32)
    assert (np.sort(idx.cpu().numpy(), axis=1) == np.sort(truth[:T], axis=1)).all()


@pytest.mark.parametrize("E,H,k,G,KG", SHAPES)
@pytest.mark.parametrize("T", TOKENS)
def test_ops_moe_router_sigmoid(E, H, k, G, KG, T):
    """ops.moe_router_sigmoid (at::linear in fp32 above T = 16): the reference's triple in the reference's order, checks 1, 2, 4"""
    from eetq_amd.ops import moe_router_sigmoid
    x, w, bias, ref, gamma = _case(T, E, H, 2000 + T + E)
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    for renorm, scale in ((True, 2.5), (False, 1.0)):
        logits, wts, idx = moe_router_sigmoid(xd, wd, bd, k, G, KG, renorm, scale)
        assert logits.dtype == torch.float32 and wts.dtype == torch.float32 and idx.dtype == torch.int64
        assert logits.shape == (T, E) and wts.shape == (T, k) and idx.shape == (T, k)
        l32, ix = logits.cpu().numpy(), idx.cpu().numpy()
        assert (np.abs(l32.astype(np.float64) - ref) <= gamma).all()
        _check_selection(l32, bias, ix, k, G, KG)
        _check_weights(wts.cpu().numpy(), l32, ix, renorm, scale)
    logits, wts, idx = moe_router_sigmoid(xd[:0], wd, bd, k, G, KG, True, 1.0)
    assert logits.shape == (0, E) and logits.dtype == torch.float32 and wts.shape == (0, k) and idx.shape == (0, k)
    with pytest.raises(RuntimeError, match="n_group"):
        moe_router_sigmoid(xd, wd, bd, k, 7, 1, True, 1.0)


@pytest.mark.parametrize("T", [3, 16, 40])
def test_exact_ties(lib, T):
    """check 6"""
    E, H, k, G, KG = 64, 2048, 8, 4, 2
    x, w, bias = inputs(T, E, H, seed=7)
    w, bias = w.copy(), bias.copy()
    w[1::2], bias[1::2] = w[0::2], bias[0::2]       # every odd expert repeats the even one before it: equal c, the lower id first
    xd = _dev(x)
    logits, idx, _, _ = _c_router(lib, xd, _dev(w), _dev(bias), k, G, KG, 1, 1.0, F32)
    l32, ix = logits.cpu().numpy(), idx.cpu().numpy()
    assert np.array_equal(l32[:, 0::2], l32[:, 1::2])
    assert (ix[:, 0::2] % 2 == 0).all() and np.array_equal(ix[:, 1::2], ix[:, 0::2] + 1)
    # all rows equal, zero bias: groups 0 .. KG-1 stay, experts in id order, equal weights
    w[:] = w[0]
    zero = torch.zeros(E, dtype=torch.float32, device=DEV)
    for renorm in (1, 0):
        logits, idx, wts, _ = _c_router(lib, xd, _dev(w), zero, k, G, KG, renorm, 2.5, F32)
        l32 = logits.cpu().numpy()
        assert (l32 == l32[:, :1]).all()
        assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(k), (T, 1)))
        s = 1.0 / (1.0 + np.exp(-l32[:, :1].astype(np.float64)))
        np.testing.assert_allclose(wts.cpu().numpy(), 2.5 * (np.full_like(s, 1.0 / k) if renorm else s) * np.ones((1, k)), rtol=2.0 ** -18)
    # four experts a group: sixteen choices span the four groups kept, in id order
    logits, idx, _, _ = _c_router(lib, xd, _dev(w), zero, 16, 16, 4, 1, 1.0, F32)
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(16), (T, 1)))


def test_equal_group_scores_go_to_the_lower_group(lib):
    """check 6, on logits written by hand: groups 1 and 2 hold the same two best values at different places, so their fp32 scores are
    equal bit for bit; with room for one of them the lower group stays"""
    E, k, G, KG = 16, 4, 4, 2
    l = np.full((3, E), -4.0, dtype=np.float32)
    l[:, 0:2] = 3.0                     # group 0: the best
    l[:, 4], l[:, 5] = 1.0, 0.5         # group 1
    l[:, 10], l[:, 9] = 1.0, 0.5        # group 2: the same two values
    l[1, 12:14] = 2.0                   # token 1: group 3 beats both, neither of the tied groups stays
    l[2, 0:2] = -4.0                    # token 2: group 0 drops out, both tied groups stay
    zero = torch.zeros(E, dtype=torch.float32, device=DEV)
    idx, wts = _c_topk(lib, _dev(l), zero, k, G, KG, 0, 1.0, F32)
    ix = idx.cpu().numpy()
    assert ix[0].tolist() == [0, 1, 4, 5]
    assert ix[1].tolist() == [0, 1, 12, 13]
    assert ix[2].tolist() == [4, 10, 5, 9]     # equal c across the two groups: the lower id first
    r = restate(l, np.zeros(E), k, G, KG, False, 1.0)
    assert np.array_equal(ix, r.idx)
    _check_weights(wts.cpu().numpy(), l, ix, 0, 1.0)


@pytest.mark.parametrize("E,H,k,G,KG", SHAPES)
@pytest.mark.parametrize("T", [1, 4, 16])
def test_fused_launch_and_selection_kernel_give_the_same_bits(lib, E, H, k, G, KG, T):
    """check 7"""
    x, w, bias, _, _ = _case(T, E, H, 31 + T)
    xd, wd = _dev(x), _dev(w)
    for bd in (_dev(bias), _dev(bias.astype(np.float16))):
        for dt, renorm, scale in ((F32, 1, 2.5), (F16, 0, 1.0)):
            logits, idx, wts, _ = _c_router(lib, xd, wd, bd, k, G, KG, renorm, scale, dt)
            idx2, wts2 = _c_topk(lib, logits, bd, k, G, KG, renorm, scale, dt)
            assert torch.equal(idx, idx2) and torch.equal(wts.view(torch.uint8), wts2.view(torch.uint8))


@pytest.mark.parametrize("E,H,k,G,KG", [s for s in SHAPES if s[1] in (512, 1024)])
@pytest.mark.parametrize("bits", [8, 4])
def test_block_ops_equal_the_layer_ops_on_the_routers_output(E, H, k, G, KG, bits):
    """check 8"""
    from eetq_amd import ops
    stacks = _experts(E, H, 384, k, bits, seed=5)
    for T in TOKENS:
        x, w, bias, _, _ = _case(T, E, H, 3000 + T)
        xd, wd, bd = _dev(x), _dev(w), _dev(bias)
        for renorm, scale in ((True, 2.5), (False, 1.0)):
            rule = (bd, k, G, KG, renorm, scale)
            routed = ops.moe_router_sigmoid(xd, wd, *rule)
            if bits == 8:
                want = ops.w8_a16_moe(xd, *routed[2:0:-1], *stacks)
                got = ops.w8_a16_moe_block_sigmoid(xd, wd, *rule, *stacks)
                assert torch.equal(got, want), (T, renorm)
                continue
            for path in ("auto", "decode", "expand"):
                want = ops.w4_a16_moe(xd, *routed[2:0:-1], *stacks, path=path)
                got = ops.w4_a16_moe_block_sigmoid(xd, wd, *rule, *stacks, path=path)
                assert torch.equal(got, want), (T, renorm, path)
        assert torch.isfinite(got).all() and got.abs().max() > 0


def test_fifty_back_to_back_launches_give_the_same_bits():
    """check 9: every launch's finishing workgroup must see every other workgroup's sums; DeepSeek-V3's own router shape"""
    from eetq_amd.ops import moe_router_sigmoid
    E, H, k, G, KG = SHAPES[1]
    x, w, bias, ref, gamma = _case(4, E, H, 11)
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    runs = [moe_router_sigmoid(xd, wd, bd, k, G, KG, True, 2.5) for _ in range(50)]
    torch.cuda.synchronize()
    assert (np.abs(runs[0][0].cpu().numpy().astype(np.float64) - ref) <= gamma).all()
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)


def test_a_softmax_router_launch_in_between_disturbs_neither():
    """check 9: the two rules share the stream's hand-over slot and ticket"""
    from eetq_amd.ops import moe_router, moe_router_sigmoid
    E, H, k, G, KG = SHAPES[1]
    x, w, bias, _, _ = _case(4, E, H, 12)
    xd, wd, bd = _dev(x), _dev(w), _dev(bias)
    x2, w2 = _softmax_inputs(7, 128, 2048, seed=13)
    x2d, w2d = _dev(x2), _dev(w2)
    alone = (moe_router_sigmoid(xd, wd, bd, k, G, KG, True, 2.5), moe_router(x2d, w2d, 8, True, torch.float32))
    torch.cuda.synchronize()
    mixed = []
    for _ in range(10):
        mixed.append((moe_router_sigmoid(xd, wd, bd, k, G, KG, True, 2.5), moe_router(x2d, w2d, 8, True, torch.float32)))
    torch.cuda.synchronize()
    for pair in mixed:
        for got, want in zip(pair, alone):
            assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("T", [4, 64])
def test_block_op_graph_replay(T):
    """check 9: a captured graph replays correctly, after a warm-up outside the capture, with replaced inputs"""
    from eetq_amd import ops
    E, H, k, G, KG = SHAPES[2]
    stacks = _experts(E, H, 384, k, 8, seed=9)
    x, w, bias, _, _ = _case(T, E, H, 77)
    x2 = _case(T, E, H, 78)[0]
    hidden, wd, bd = _dev(x), _dev(w), _dev(bias)
    args = (wd, bd, k, G, KG, True, 2.5, *stacks)
    ops.w8_a16_moe_block_sigmoid(hidden, *args)  # warm-up: the hand-over slot is created outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.w8_a16_moe_block_sigmoid(hidden, *args)
    hidden.copy_(_dev(x2))
    g.replay()
    torch.cuda.synchronize()
    fresh = ops.w8_a16_moe_block_sigmoid(_dev(x2), *args)
    assert torch.equal(out, fresh)
    assert not torch.equal(fresh, ops.w8_a16_moe_block_sigmoid(_dev(x), *args))


@pytest.mark.parametrize("kind", ["deepseek_v3", "glm4_moe"])
def test_models_with_and_without_the_device_router(kind):
    """check 10"""
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter
    from eetq_amd.utils.quantizer import eet_quantize
    torch.manual_seed(3)
    base = tiny(kind).half().to(DEV).eval()
    with torch.no_grad():
        for layer in base.model.layers[1:]:
            layer.mlp.gate.weight.normal_(0, 0.5)
            layer.mlp.gate.e_score_correction_bias.uniform_(-0.25, 0.25)
    plain, routed = copy.deepcopy(base), copy.deepcopy(base)
    eet_quantize(plain, experts=True)
    eet_quantize(routed, experts=True, router=True)
    sparse = routed.model.layers[1:]
    assert all(isinstance(l.mlp, EetqSparseMoeBlock) and isinstance(l.mlp.gate, EetqTopKRouter) for l in sparse)
    assert not any(isinstance(m, (EetqSparseMoeBlock, EetqTopKRouter)) for m in plain.modules())
    ids = torch.randint(0, 256, (2, 7), device=DEV)
    seen = {}

    def hook(tag):
        return lambda mod, args, out: seen.__setitem__(tag, (args[0].detach().reshape(-1, 128).cpu().numpy(), out[0].cpu().numpy()))
    h1 = plain.model.layers[1].mlp.gate.register_forward_hook(hook("plain"))
    h2 = routed.model.layers[1].mlp.gate.register_forward_hook(hook("routed"))
    with torch.no_grad():
        a = plain(ids).logits
        b = routed(ids).logits      # the first sparse layer is observed (unfused, device router); the second runs the block op
    h1.remove()
    h2.remove()
    assert np.array_equal(seen["plain"][0], seen["routed"][0])           # the first MoE block's input is the same in both
    ref, gamma = ref_logits(seen["plain"][0], routed.model.layers[1].mlp.gate.weight.detach().cpu().numpy())
    for tag in ("plain", "routed"):
        assert seen[tag][1].dtype == np.float32
        _check_logits(seen[tag][1], ref, gamma)
    hooks = [l.mlp.gate.register_forward_hook(lambda m, i, o: None) for l in sparse]
    with torch.no_grad():
        assert not any(l.mlp.fused(torch.zeros(1, 1, 128, device=DEV, dtype=torch.float16)) for l in sparse)
        observed = routed(ids).logits      # every gate observed: every block on the unfused path
    for h in hooks:
        h.remove()
    h3 = routed.model.layers[2].mlp.shared_experts.register_forward_hook(lambda m, i, o: None)
    with torch.no_grad():
        shared_observed = routed(ids).logits
    h3.remove()
    with torch.no_grad():
        assert all(l.mlp.fused(torch.zeros(1, 1, 128, device=DEV, dtype=torch.float16)) for l in sparse)
        c = routed(ids).logits      # no hooks: both sparse layers run the block op + the shared expert
        d = routed(ids).logits
        one = routed(ids[:1, :1]).logits
    for t in (a, b, c, one):
        assert torch.isfinite(t).all()
    assert torch.equal(c, d)
    assert torch.equal(observed, c) and torch.equal(b, c) and torch.equal(shared_observed, c)   # the bits of the unfused path
    # a call that needs gradients reaches the original forward: the unswapped router's gradients
    gate, ref_gate = routed.model.layers[1].mlp.gate, base.model.layers[1].mlp.gate
    grads = []
    for g in (gate, ref_gate):
        x = torch.randn(5, 128, device=DEV, dtype=torch.float16, generator=torch.Generator(DEV).manual_seed(1)).requires_grad_(True)
        g.weight.grad = None
        logits, wts, idx = g(x)
        (wts.float().sum() + logits.float().pow(2).sum()).backward()
        grads.append((x.grad.clone(), g.weight.grad.clone(), idx))
    assert all(torch.equal(p, q) for p, q in zip(*grads))
    assert grads[0][0].abs().max() > 0
