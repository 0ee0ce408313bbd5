"""The device MoE router's surface without a GPU: the two C entries are declared, exported and refuse bad
arguments before any device work; the ctypes binding refuses the ops by name; eet_quantize(experts=True, router=True) converts
exactly the allow-listed routers and blocks in place, with unchanged state-dict keys, leaves a Qwen2-MoE block (shared expert) a
Qwen2-MoE block with a device router, needs experts=True, and by default touches no router and no block."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eetq_moe_router_f16", "eetq_moe_topk_f16")
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
F16, F32 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_error_codes_and_dtypes_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name, val in (("EETQ_ERR_INVALID", ERR_INVALID), ("EETQ_ERR_UNSUPPORTED", ERR_UNSUPPORTED), ("EETQ_DTYPE_F16", F16),
                      ("EETQ_DTYPE_F32", F32)):
        m = re.search(r"%s\s*=?\s*\(?(-?\d+)\)?" % name, hdr)
        assert m and int(m.group(1)) == val, name


def test_router_entries_declared_and_exported(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "TopKRouter" in hdr                      # the header cites what the entries replace
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr
    assert lib.eetq_abi_version() == 7
    mk = open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()
    assert "moe_router.hip" in mk and re.search(r"HAZARD_CHECKED\s*:=.*moe_router\.o", mk)


def test_router_rejects_bad_arguments_without_a_device(lib):
    p, n = ctypes.c_void_p(4096), None  # never dereferenced: every case fails its argument check first
    f = lib.eetq_moe_router_f16
    #     x  w  T  H     E  k  rn dt   logits idx wts counts off sorted pos active stream
    ok = (p, p, 4, 2048, 8, 2, 1, F32, p, p, p, p, p, p, p, p, n)

    def call(**kw):
        names = ("x", "w", "T", "H", "E", "k", "renorm", "w_dtype", "logits", "idx", "wts", "counts", "offsets", "sorted", "position",
                 "active", "stream")
        args = list(ok)
        for key, v in kw.items():
            args[names.index(key)] = v
        return f(*args)

    for name in ("x", "w", "logits", "idx", "wts"):
        assert call(**{name: n}) == ERR_INVALID, name
        assert b"null pointer" in lib.eetq_last_error()
    for name in ("counts", "offsets", "sorted", "position", "active"):      # tables half null
        assert call(**{name: n}) == ERR_INVALID, name
        assert b"all null or all set" in lib.eetq_last_error()
    assert call(E=0) == ERR_INVALID
    assert call(E=257, k=2) == ERR_UNSUPPORTED and b"E <= 256" in lib.eetq_last_error()
    assert call(E=64, k=17) == ERR_UNSUPPORTED
    assert call(k=0) == ERR_INVALID
    assert call(k=9) == ERR_INVALID                                          # k > E
    assert call(T=0) == ERR_INVALID and call(T=-1) == ERR_INVALID
    assert call(H=2000) == ERR_INVALID and b"multiple of 64" in lib.eetq_last_error()
    assert call(H=0) == ERR_INVALID
    assert call(w_dtype=7) == ERR_INVALID and b"fp16 or fp32" in lib.eetq_last_error()
    assert call(renorm=2) == ERR_INVALID
    assert call(x=ctypes.c_void_p(4104)) == ERR_INVALID and b"16-byte" in lib.eetq_last_error()
    assert call(w=ctypes.c_void_p(4104)) == ERR_INVALID
    assert call(T=17, H=100) == ERR_INVALID                                  # the same checks above the fused launch's T


def test_topk_rejects_bad_arguments_without_a_device(lib):
    p, n = ctypes.c_void_p(4096), None
    f = lib.eetq_moe_topk_f16
    assert f(n, 4, 8, 2, 1, F32, p, p, n) == ERR_INVALID
    assert f(p, 4, 8, 2, 1, F32, n, p, n) == ERR_INVALID
    assert f(p, 4, 8, 2, 1, F32, p, n, n) == ERR_INVALID
    assert f(p, 0, 8, 2, 1, F32, p, p, n) == ERR_INVALID
    assert f(p, 4, 0, 2, 1, F32, p, p, n) == ERR_INVALID
    assert f(p, 4, 300, 2, 1, F32, p, p, n) == ERR_UNSUPPORTED
    assert f(p, 4, 8, 0, 1, F32, p, p, n) == ERR_INVALID
    assert f(p, 4, 8, 9, 1, F32, p, p, n) == ERR_INVALID
    assert f(p, 4, 8, 2, 1, 5, p, p, n) == ERR_INVALID
    assert f(p, 4, 8, 2, 3, F16, p, p, n) == ERR_INVALID


def test_ctypes_binding_refuses_the_router_ops_by_name():
    from eetq_amd import ops_ctypes
    for name, nargs in (("moe_router", 3), ("w8_a16_moe_block", 9), ("w4_a16_moe_block", 9)):
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
    for name in ("moe_router", "w8_a16_moe_block", "w4_a16_moe_block"):
        assert name in ops.__all__ and callable(getattr(ops, name))


def _mixtral():
    from transformers import MixtralConfig, MixtralForCausalLM
    cfg = MixtralConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=8, num_experts_per_tok=2, vocab_size=256)
    return MixtralForCausalLM(cfg).half()


def _qwen3_moe():
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    cfg = Qwen3MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=128, num_hidden_layers=2,
                         num_attention_heads=4, num_key_value_heads=2, num_experts=16, num_experts_per_tok=4, vocab_size=256,
                         decoder_sparse_step=1, mlp_only_layers=[])
    return Qwen3MoeForCausalLM(cfg).half()


def _olmoe():
    from transformers import OlmoeConfig, OlmoeForCausalLM
    cfg = OlmoeConfig(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      num_experts=16, num_experts_per_tok=4, vocab_size=256)
    return OlmoeForCausalLM(cfg).half()


def _qwen2_moe():
    from transformers import Qwen2MoeConfig, Qwen2MoeForCausalLM
    cfg = Qwen2MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=128, shared_expert_intermediate_size=128,
                         num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, num_experts=16, num_experts_per_tok=4,
                         vocab_size=256, decoder_sparse_step=1, mlp_only_layers=[])
    return Qwen2MoeForCausalLM(cfg).half()


def _keys(model):
    """the state-dict keys (taking state_dict() itself re-encodes the int8 buffers, which needs a device)"""
    return sorted([n for n, _ in model.named_parameters()] + [n for n, b in model.named_buffers() if b is not None])


def _types(model):
    return {n: type(m).__name__ for n, m in model.named_modules()}


@pytest.mark.parametrize("make,router,block,bits", [(_mixtral, "MixtralTopKRouter", "MixtralSparseMoeBlock", 8),
                                                    (_qwen3_moe, "Qwen3MoeTopKRouter", "Qwen3MoeSparseMoeBlock", 8),
                                                    (_olmoe, "OlmoeTopKRouter", "OlmoeSparseMoeBlock", 4)])
def test_router_true_swaps_exactly_the_listed_classes(make, router, block, bits):
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter, W4A16Experts, W8A16Experts
    from eetq_amd.utils.quantizer import eet_quantize
    model, plain = make(), make()
    before = _types(model)
    eet_quantize(plain, init_only=True, experts=True, expert_bits=bits)
    eet_quantize(model, init_only=True, experts=True, expert_bits=bits, router=True)
    after = _types(model)
    assert list(after) == list(_types(plain))               # next to experts=True alone: no module appeared, vanished or moved
    assert _keys(model) == _keys(plain)
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in plain.named_parameters()]
    swapped = {n for n in after if after[n] in ("EetqTopKRouter", "EetqSparseMoeBlock")}
    assert swapped == {n for n, t in before.items() if t in (router, block)} and len(swapped) == 4
    assert _types(plain) == {n: (before[n] if n in swapped else t) for n, t in after.items()}   # nothing else differs
    for layer in model.model.layers:
        mlp = layer.mlp
        assert isinstance(mlp, EetqSparseMoeBlock) and type(mlp).__mro__[2].__name__ == block   # still its original class
        assert isinstance(mlp.gate, EetqTopKRouter) and type(mlp.gate).__mro__[2].__name__ == router
        assert isinstance(mlp.experts, W4A16Experts if bits == 4 else W8A16Experts)
        assert isinstance(mlp.gate.weight, torch.nn.Parameter) and mlp.gate.weight.shape == (mlp.gate.num_experts, 128)
        assert mlp.gate.renormalises == (True if router.startswith("Mixtral") else bool(mlp.gate.norm_topk_prob))
        assert mlp.gate.scores_dtype() == (torch.float32 if router.startswith("Mixtral") else torch.float16)


def test_qwen2_moe_keeps_its_block_and_gets_the_router():
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter, W8A16Experts
    from eetq_amd.utils.quantizer import eet_quantize
    model = _qwen2_moe()
    keys = _keys(model)
    eet_quantize(model, init_only=True, experts=True, router=True)
    for layer in model.model.layers:
        assert type(layer.mlp).__name__ == "Qwen2MoeSparseMoeBlock" and not isinstance(layer.mlp, EetqSparseMoeBlock)
        assert isinstance(layer.mlp.gate, EetqTopKRouter) and isinstance(layer.mlp.experts, W8A16Experts)
    gate_keys = {k for k in keys if ".mlp.gate." in k}
    assert len(gate_keys) == 2 and gate_keys <= set(_keys(model))


def test_an_unlisted_router_is_named_in_the_one_warning():
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()

    class OtherRouter(type(model.model.layers[1].mlp.gate)):
        pass
    model.model.layers[1].mlp.gate.__class__ = OtherRouter
    with pytest.warns(UserWarning, match="1 router") as rec:
        eet_quantize(model, init_only=True, experts=True, router=True)
    msgs = [str(w.message) for w in rec if "eet_quantize" in str(w.message)]
    assert len(msgs) == 1 and "layers.1.mlp.gate" in msgs[0] and "OtherRouter" in msgs[0]
    assert type(model.model.layers[0].mlp).__name__ == "EetqSparseMoeBlock"
    assert type(model.model.layers[1].mlp).__name__ == "MixtralSparseMoeBlock" and type(model.model.layers[1].mlp.gate) is OtherRouter


def test_router_needs_experts_and_raises_before_the_model_is_touched():
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()
    before = [(n, type(m), id(m)) for n, m in model.named_modules()]
    with pytest.raises(ValueError, match="router=True needs experts=True"):
        eet_quantize(model, init_only=True, router=True)
    assert [(n, type(m), id(m)) for n, m in model.named_modules()] == before


@pytest.mark.parametrize("make", [_mixtral, _qwen3_moe, _olmoe, _qwen2_moe])
def test_default_leaves_every_router_and_block(make):
    import inspect

    from eetq_amd.utils.quantizer import eet_quantize
    params = list(inspect.signature(eet_quantize).parameters.values())
    assert params[-1].name == "router" and params[-1].default is False
    model = make()
    before = _types(model)
    eet_quantize(model, init_only=True, experts=True)
    after = _types(model)
    for n, t in before.items():
        if "Router" in t or "SparseMoeBlock" in t:
            assert after[n] == t, n
    assert not any(t.startswith("Eetq") for t in after.values())


def test_fallback_rules_without_a_device():
    """which calls take the torch forward is decided from grad mode, flags and hooks alone"""
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()
    eet_quantize(model, init_only=True, experts=True, router=True)
    mlp = model.model.layers[0].mlp
    x = torch.zeros(1, 2, 128, dtype=torch.float16)
    assert mlp.gate.falls_back(x) and not mlp.fused(x)          # grad mode on, the router weight requires grad
    with torch.no_grad():
        assert not mlp.gate.falls_back(x) and mlp.fused(x)
        h = mlp.gate.register_forward_hook(lambda m, a, o: None)  # what output_router_logits=True installs
        assert not mlp.fused(x)
        h.remove()
        assert mlp.fused(x)
        mlp.jitter_noise, mlp.training = 0.1, True
        assert not mlp.fused(x)
        mlp.training = False
        assert mlp.fused(x)
    mlp.gate.weight.requires_grad_(False)
    assert not mlp.gate.falls_back(x) and mlp.fused(x)
    assert mlp.gate.falls_back(x.clone().requires_grad_(True))
    mlp.experts.trainable = True
    assert not mlp.fused(x)
    with torch.no_grad():
        assert mlp.fused(x)
    # the fallback IS the original forward: on the CPU, in fp32, it equals the unswapped router's
    ref = _mixtral().float()
    ref.model.layers[0].mlp.gate.weight.data.copy_(mlp.gate.weight.data.float())
    gate = mlp.gate.float()
    gate.weight.requires_grad_(True)
    xs = torch.randn(5, 128)
    for a, b in zip(gate(xs), ref.model.layers[0].mlp.gate(xs)):
        assert torch.equal(a, b)
