"""The sigmoid, bias-corrected, group-limited device router's surface without a GPU: the two C entries are declared,
exported and refuse bad arguments before any device work; the ctypes binding refuses the three ops by name; eet_quantize(experts=True,
router=True) converts exactly the routers and blocks of tiny DeepSeek-V3 and GLM-4-MoE models in place, with unchanged module names
and parameter / buffer keys and without a warning, names a router whose groups the kernel does not serve, and decides the fallback
from grad mode, flags and hooks alone; and the float64 restatement of the contract that the GPU tests check the kernels against
agrees with transformers' own router on the CPU.

restate() is that restatement.  DELTA = 2^-21 bounds the error of an fp32 score for choice c = sigmoid(logit) + bias against its
float64 value at |c| <= 1.25: exp, the division and the add each contribute at most a few ulps of 2^-24 .. 2^-23."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eetq_moe_router_sigmoid_f16", "eetq_moe_topk_sigmoid_f32")
OPS = ("moe_router_sigmoid", "w8_a16_moe_block_sigmoid", "w4_a16_moe_block_sigmoid")
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
F16, F32 = 0, 1
DELTA = 2.0 ** -21
# (E, H, k, G, KG)
SHAPES = [(256, 512, 8, 8, 4), (256, 7168, 8, 8, 4), (160, 1024, 6, 8, 3), (128, 2048, 8, 1, 1), (16, 128, 4, 4, 2), (64, 2048, 8, 4, 4)]


def inputs(T, E, H, seed):
    """fp16 x [T, H], w [E, H] with max|logit| = 5 (as the softmax router's tests) and an fp32 bias [E] uniform in +-0.25"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, H)).astype(np.float16)
    w = (rng.standard_normal((E, H)) / np.sqrt(H)).astype(np.float16)
    w = (w.astype(np.float64) * (5.0 / np.abs(x.astype(np.float64) @ w.astype(np.float64).T).max())).astype(np.float16)
    bias = rng.uniform(-0.25, 0.25, E).astype(np.float32)
    return x, w, bias


def ref_logits(x, w):
    """float64 logits of the fp16 inputs and gamma = H 2^-24 sum_h |x_h w_eh|: the worst-case error of an fp32 summation of H exact
    products in any order (no rounding to fp16 follows)"""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    return x64 @ w64.T, x.shape[1] * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64).T)


class Restated:
    pass


def restate(logits, bias, k, G, KG, renorm=True, scale=1.0):
    """The contract in float64 on `logits` [T, E]: .s, .c [T, E]; .gscore [T, G]; .kept [T, G] bool; .idx [T, k] (descending c, ties
    to the lower id); .weights [T, k]; .gmargin [T] (KG-th minus (KG+1)-th group score, inf when all groups stay); .emargin [T]
    (k-th minus (k+1)-th c among the kept experts, inf when there is no (k+1)-th)."""
    r = Restated()
    l = np.asarray(logits, dtype=np.float64)
    T, E = l.shape
    per = E // G
    r.s = 1.0 / (1.0 + np.exp(-l))
    r.c = r.s + np.asarray(bias, dtype=np.float64)
    if G > 1:
        r.gscore = np.sort(r.c.reshape(T, G, per), axis=2)[:, :, -2:].sum(axis=2)
    else:
        r.gscore = np.zeros((T, 1))
    gorder = np.argsort(-r.gscore, axis=1, kind="stable")
    r.kept = np.zeros((T, G), dtype=bool)
    np.put_along_axis(r.kept, gorder[:, :KG], True, axis=1)
    gsorted = np.take_along_axis(r.gscore, gorder, axis=1)
    r.gmargin = gsorted[:, KG - 1] - gsorted[:, KG] if KG < G else np.full(T, np.inf)
    r.kth_gscore = gsorted[:, KG - 1]
    masked = np.where(np.repeat(r.kept, per, axis=1), r.c, -np.inf)
    order = np.argsort(-masked, axis=1, kind="stable")
    r.idx = order[:, :k]
    csorted = np.take_along_axis(masked, order, axis=1)
    r.emargin = csorted[:, k - 1] - csorted[:, k] if k < KG * per else np.full(T, np.inf)
    r.weights = weights64(l, r.idx, renorm, scale)
    return r


def weights64(logits, idx, renorm, scale):
    """the weights of the contract at given indices: the sigmoid without the bias, renormalised over the selection, scaled"""
    s = np.take_along_axis(1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64))), idx, axis=1)
    if renorm:
        s = s / (s.sum(axis=1, keepdims=True) + 1e-20)
    return s * scale


def separated(r, group_slack, expert_slack):
    return (r.gmargin > group_slack) & (r.emargin > expert_slack)


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_entries_declared_and_exported(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "DeepseekV3TopkRouter" in hdr and "e_score_correction_bias" in hdr
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr
    assert lib.eetq_abi_version() == 7
    mk = open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()
    assert re.search(r"HAZARD_CHECKED\s*:=.*moe_router\.o", mk)


def test_router_rejects_bad_arguments_without_a_device(lib):
    p, n = ctypes.c_void_p(4096), None  # never dereferenced: every case fails its argument check first
    names = ("x", "w", "bias", "bias_dtype", "T", "H", "E", "k", "n_group", "topk_group", "renorm", "scale", "w_dtype", "logits", "idx",
             "wts", "counts", "offsets", "sorted", "position", "active", "stream")
    ok = (p, p, p, F32, 4, 2048, 16, 4, 4, 2, 1, 2.5, F32, p, p, p, p, p, p, p, p, n)

    def call(**kw):
        args = list(ok)
        for key, v in kw.items():
            args[names.index(key)] = v
        return lib.eetq_moe_router_sigmoid_f16(*args)

    for name in ("x", "w", "bias", "logits", "idx", "wts"):
        assert call(**{name: n}) == ERR_INVALID, name
        assert b"null pointer" in lib.eetq_last_error()
    for name in ("counts", "offsets", "sorted", "position", "active"):
        assert call(**{name: n}) == ERR_INVALID, name
    assert call(n_group=3) == ERR_INVALID and b"multiple of n_group" in lib.eetq_last_error()       # E % G
    assert call(n_group=16, topk_group=8) == ERR_INVALID and b"two experts" in lib.eetq_last_error()   # E / G < 2
    assert call(topk_group=5) == ERR_INVALID and call(topk_group=0) == ERR_INVALID                    # KG > G
    assert call(topk_group=1, k=5) == ERR_INVALID and b"kept groups" in lib.eetq_last_error()          # k > KG E / G
    assert call(n_group=0) == ERR_INVALID
    assert call(E=257, n_group=1, topk_group=1) == ERR_UNSUPPORTED and b"E <= 256" in lib.eetq_last_error()
    assert call(E=64, k=17, n_group=1, topk_group=1) == ERR_UNSUPPORTED
    assert call(E=256, n_group=128, topk_group=128) == ERR_UNSUPPORTED and b"n_group <= 64" in lib.eetq_last_error()
    assert call(H=2000) == ERR_INVALID and b"multiple of 64" in lib.eetq_last_error()                  # H % 64
    assert call(bias_dtype=7) == ERR_INVALID and b"bias must be fp16 or fp32" in lib.eetq_last_error()
    assert call(w_dtype=7) == ERR_INVALID and call(renorm=2) == ERR_INVALID
    assert call(scale=float("inf")) == ERR_INVALID and call(scale=float("nan")) == ERR_INVALID
    assert call(k=0) == ERR_INVALID and call(T=0) == ERR_INVALID
    assert call(x=ctypes.c_void_p(4104)) == ERR_INVALID and b"16-byte" in lib.eetq_last_error()
    assert call(T=17, n_group=3) == ERR_INVALID                                                       # the same checks above the fused T


def test_topk_rejects_bad_arguments_without_a_device(lib):
    p, n = ctypes.c_void_p(4096), None
    names = ("logits", "bias", "bias_dtype", "T", "E", "k", "n_group", "topk_group", "renorm", "scale", "w_dtype", "idx", "wts", "stream")
    ok = (p, p, F16, 4, 16, 4, 4, 2, 1, 1.0, F32, p, p, n)

    def call(**kw):
        args = list(ok)
        for key, v in kw.items():
            args[names.index(key)] = v
        return lib.eetq_moe_topk_sigmoid_f32(*args)

    for name in ("logits", "bias", "idx", "wts"):
        assert call(**{name: n}) == ERR_INVALID, name
    assert call(n_group=3) == ERR_INVALID and call(n_group=16, topk_group=8) == ERR_INVALID
    assert call(topk_group=5) == ERR_INVALID and call(topk_group=1, k=5) == ERR_INVALID
    assert call(E=257, n_group=1, topk_group=1) == ERR_UNSUPPORTED and call(E=64, k=17, n_group=1, topk_group=1) == ERR_UNSUPPORTED
    assert call(bias_dtype=2) == ERR_INVALID and call(w_dtype=5) == ERR_INVALID and call(T=0) == ERR_INVALID


def test_ctypes_binding_refuses_the_sigmoid_ops_by_name():
    from eetq_amd import ops_ctypes
    for name, nargs in zip(OPS, (8, 12, 12)):
        assert name in ops_ctypes.__all__
        with pytest.raises(RuntimeError, match=name + " needs the compiled EETQ module"):
            getattr(ops_ctypes, name)(*([None] * nargs))


def test_exports():
    import eetq
    import eetq_amd
    import eetq_amd.modules
    from eetq_amd import ops
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter
    for cls in (EetqTopKRouter, EetqSparseMoeBlock):
        assert getattr(eetq_amd, cls.__name__) is cls and getattr(eetq_amd.modules, cls.__name__) is cls
        assert getattr(eetq, cls.__name__) is cls
    for name in OPS:
        assert name in ops.__all__ and callable(getattr(ops, name))
    assert set(EetqTopKRouter.SIGMOID_CLASS_NAMES) == {"DeepseekV3TopkRouter", "DeepseekV32TopkRouter", "Glm4MoeTopkRouter",
                                                       "Glm4MoeLiteTopkRouter", "Dots1TopkRouter", "SolarOpenTopkRouter"}
    assert set(EetqTopKRouter.SIGMOID_CLASS_NAMES) <= set(EetqTopKRouter.CLASS_NAMES)
    assert set(EetqSparseMoeBlock.SHARED_CLASS_NAMES) == {"DeepseekV3MoE", "DeepseekV32MoE", "Glm4MoeMoE", "Glm4MoeLiteMoE", "Dots1MoE",
                                                          "SolarOpenMoE"}


def tiny(kind, n_group=4):
    """hidden 128, 16 routed experts, k 4, G 4, KG 2, one dense and two sparse layers"""
    import transformers as tf
    common = dict(hidden_size=128, intermediate_size=256, moe_intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
                  n_routed_experts=16, num_experts_per_tok=4, n_group=n_group, topk_group=2, n_shared_experts=1, first_k_dense_replace=1,
                  vocab_size=256, norm_topk_prob=True, attn_implementation="eager")
    if kind == "deepseek_v3":
        cfg = tf.DeepseekV3Config(num_key_value_heads=4, q_lora_rank=64, kv_lora_rank=64, qk_rope_head_dim=16, qk_nope_head_dim=16,
                                  v_head_dim=32, routed_scaling_factor=2.5, **common)
        return tf.DeepseekV3ForCausalLM(cfg)
    cfg = tf.Glm4MoeConfig(num_key_value_heads=2, head_dim=32, routed_scaling_factor=1.0, **common)
    return tf.Glm4MoeForCausalLM(cfg)


def _keys(model):
    return sorted([n for n, _ in model.named_parameters()] + [n for n, b in model.named_buffers() if b is not None])


def _types(model):
    return {n: type(m).__name__ for n, m in model.named_modules()}


@pytest.mark.parametrize("kind,router,block,bits", [("deepseek_v3", "DeepseekV3TopkRouter", "DeepseekV3MoE", 8),
                                                    ("glm4_moe", "Glm4MoeTopkRouter", "Glm4MoeMoE", 4)])
def test_router_true_swaps_exactly_the_routers_and_blocks(kind, router, block, bits):
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter, W4A16Experts, W8A16Experts, W8A16Linear
    from eetq_amd.utils.quantizer import eet_quantize
    torch.manual_seed(0)
    model, plain = tiny(kind).half(), tiny(kind).half()
    before = _types(model)
    eet_quantize(plain, init_only=True, experts=True, expert_bits=bits)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        eet_quantize(model, init_only=True, experts=True, expert_bits=bits, router=True)
    assert not [str(w.message) for w in rec if "left on torch" in str(w.message) or "left in fp16" in str(w.message)]
    after = _types(model)
    assert list(after) == list(_types(plain))     # next to experts=True alone: no module appeared, vanished, moved or was renamed
    assert _keys(model) == _keys(plain)
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert sum(k.endswith("gate.e_score_correction_bias") for k in _keys(model)) == 2
    swapped = {n for n in after if after[n] in ("EetqTopKRouter", "EetqSparseMoeBlock")}
    assert swapped == {n for n, t in before.items() if t in (router, block)} and len(swapped) == 4
    assert _types(plain) == {n: (before[n] if n in swapped else t) for n, t in after.items()}   # nothing else differs
    assert type(model.model.layers[0].mlp).__name__.endswith("MLP")                              # the dense layer
    for layer in model.model.layers[1:]:
        mlp = layer.mlp
        assert isinstance(mlp, EetqSparseMoeBlock) and type(mlp).__mro__[2].__name__ == block   # still its original class
        assert isinstance(mlp.gate, EetqTopKRouter) and type(mlp.gate).__mro__[2].__name__ == router
        assert mlp.gate.is_sigmoid and mlp.gate.scores_dtype() == torch.float32
        assert isinstance(mlp.experts, W4A16Experts if bits == 4 else W8A16Experts)
        assert all(isinstance(getattr(mlp.shared_experts, p), W8A16Linear) for p in ("gate_proj", "up_proj", "down_proj"))
        bias = mlp.gate.e_score_correction_bias
        assert bias.shape == (16,) and bias.dtype == torch.float16 and "e_score_correction_bias" in dict(mlp.gate.named_buffers())
        assert mlp.gate.sigmoid_args()[1:] == (4, 4, 2, True, 2.5 if kind == "deepseek_v3" else 1.0)


def test_a_router_with_groups_the_kernel_does_not_serve_is_named_and_stays():
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter
    from eetq_amd.utils.quantizer import eet_quantize
    model = tiny("deepseek_v3").half()
    model.model.layers[2].mlp.gate.num_group = 3      # 16 experts do not divide into 3 groups
    with pytest.warns(UserWarning, match="1 router") as rec:
        eet_quantize(model, init_only=True, experts=True, router=True)
    msgs = [str(w.message) for w in rec if "eet_quantize" in str(w.message)]
    assert len(msgs) == 1 and "layers.2.mlp.gate" in msgs[0] and "n_group = 3" in msgs[0] and "layers.1" not in msgs[0]
    assert isinstance(model.model.layers[1].mlp, EetqSparseMoeBlock)
    assert type(model.model.layers[2].mlp).__name__ == "DeepseekV3MoE" and type(model.model.layers[2].mlp.gate).__name__ == "DeepseekV3TopkRouter"
    # every attribute the forward reads is required, and every limit has its reason
    gate = tiny("deepseek_v3").half().model.layers[1].mlp.gate
    assert EetqTopKRouter.unsupported_reason(gate) is None
    for attr in ("num_group", "topk_group", "norm_topk_prob", "routed_scaling_factor"):
        keep = getattr(gate, attr)
        delattr(gate, attr)
        assert attr in EetqTopKRouter.unsupported_reason(gate)
        setattr(gate, attr, keep)
    keep = gate._buffers.pop("e_score_correction_bias")
    assert "e_score_correction_bias" in EetqTopKRouter.unsupported_reason(gate)
    gate.register_buffer("e_score_correction_bias", keep.double())
    assert "float16 or float32" in EetqTopKRouter.unsupported_reason(gate)
    gate.e_score_correction_bias = keep
    for attr, bad in (("num_group", 16), ("topk_group", 5), ("topk_group", 0), ("top_k", 9), ("top_k", 17), ("routed_scaling_factor", float("inf"))):
        keep = getattr(gate, attr)
        setattr(gate, attr, bad)
        assert EetqTopKRouter.unsupported_reason(gate) is not None, (attr, bad)
        setattr(gate, attr, keep)
    assert EetqTopKRouter.unsupported_reason(gate) is None


def test_fallback_and_hook_rules_without_a_device():
    from eetq_amd.utils.quantizer import eet_quantize
    torch.manual_seed(1)
    model = tiny("deepseek_v3").half()
    eet_quantize(model, init_only=True, experts=True, router=True)
    mlp = model.model.layers[1].mlp
    x = torch.zeros(1, 2, 128, dtype=torch.float16)
    assert mlp.gate.falls_back(x) and not mlp.fused(x)          # grad mode on, the router weight requires grad
    with torch.no_grad():
        assert not mlp.gate.falls_back(x) and mlp.fused(x)
        for sub in (mlp.gate, mlp.experts, mlp.shared_experts):
            h = sub.register_forward_hook(lambda m, a, o: None)
            assert not mlp.fused(x)
            h.remove()
            assert mlp.fused(x)
        h = mlp.shared_experts.register_forward_pre_hook(lambda m, a: None)
        assert not mlp.fused(x)
        h.remove()
    mlp.gate.weight.requires_grad_(False)
    assert not mlp.gate.falls_back(x) and mlp.fused(x)
    assert mlp.gate.falls_back(x.clone().requires_grad_(True))
    mlp.experts.trainable = True
    assert not mlp.fused(x)
    with torch.no_grad():
        assert mlp.fused(x)
    # the fallback IS the original forward: on the CPU, in fp32, it equals the unswapped router's
    ref = tiny("deepseek_v3").model.layers[1].mlp.gate
    gate = mlp.gate.float()
    ref.weight.data.copy_(gate.weight.data)
    ref.e_score_correction_bias.copy_(gate.e_score_correction_bias)
    gate.weight.requires_grad_(True)
    xs = torch.randn(5, 128)
    for a, b in zip(gate(xs), ref(xs)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("E,H,k,G,KG", [s for s in SHAPES if s[1] <= 2048] + [(64, 2048, 6, 1, 1)])
@pytest.mark.parametrize("renorm,scale", [(True, 2.5), (False, 1.0)])
def test_restatement_agrees_with_transformers_router(E, H, k, G, KG, renorm, scale):
    """transformers' DeepseekV3TopkRouter on an fp16 model on the CPU against restate() on the router's own fp32 logits: the same
    index sets on every separated token (group margin > 8 delta, expert margin > 2 delta: the reference's c is fp32 too), weights
    within 2^-18 relative (the project's budget for an fp32 score), logits within gamma of the float64 ones"""
    import transformers as tf
    from transformers.models.deepseek_v3.modeling_deepseek_v3 import DeepseekV3TopkRouter
    T = 32
    x, w, bias = inputs(T, E, H, seed=100 + E + k)
    cfg = tf.DeepseekV3Config(hidden_size=H, n_routed_experts=E, num_experts_per_tok=k, n_group=G, topk_group=KG,
                              norm_topk_prob=renorm, routed_scaling_factor=scale)
    gate = DeepseekV3TopkRouter(cfg).half()
    with torch.no_grad():
        gate.weight.copy_(torch.from_numpy(w))
        gate.e_score_correction_bias.copy_(torch.from_numpy(bias))
        logits, weights, idx = gate(torch.from_numpy(x))
    assert logits.dtype == torch.float32 and weights.dtype == torch.float32 and idx.dtype == torch.int64
    ref, gamma = ref_logits(x, w)
    assert (np.abs(logits.numpy().astype(np.float64) - ref) <= gamma).all()
    bias16 = gate.e_score_correction_bias.numpy()      # the buffer is fp16 after .half(): the kernel's bias_dtype flag
    assert bias16.dtype == np.float16
    r = restate(logits.numpy(), bias16, k, G, KG, renorm, scale)
    sep = separated(r, 8 * DELTA, 2 * DELTA)
    print("separated %d / %d, smallest margins: group %.3g, expert %.3g" % (sep.sum(), T, r.gmargin.min(), r.emargin.min()))
    assert sep.mean() >= 0.95
    ix = idx.numpy()
    assert (np.sort(ix[sep], axis=1) == np.sort(r.idx[sep], axis=1)).all()
    want = weights64(logits.numpy(), ix, renorm, scale)
    rel = np.abs(weights.numpy().astype(np.float64) - want) / want
    print("weights: max relative error %.3g" % rel.max())
    assert rel.max() <= 2.0 ** -18
