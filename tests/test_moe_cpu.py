"""Mixture-of-experts surface without a GPU: the routed-expert C entries are declared, exported and refuse bad arguments before
any launch; eet_quantize(experts=True) swaps transformers' 3-D experts modules for W8A16Experts (init_only: buffers only) and
leaves them alone by default; from_experts rejects the expert forms it cannot run."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eetq_moe_route", "eetq_w8a16_moe_gemm", "eetq_moe_combine_f16")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_moe_entries_declared_and_exported(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr
    assert "moe.hip" in open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()


def test_moe_entries_reject_bad_arguments_without_a_device(lib):
    p = ctypes.c_void_p(16)  # never dereferenced: every case fails its argument check first
    n = None
    # route: null pointer, E out of range, k out of range, T < 1
    assert lib.eetq_moe_route(n, 4, 2, 8, p, p, p, p, p, n) == ERR_INVALID
    assert lib.eetq_moe_route(p, 4, 2, 0, p, p, p, p, p, n) == ERR_INVALID
    assert lib.eetq_moe_route(p, 4, 2, 1025, p, p, p, p, p, n) == ERR_INVALID
    assert lib.eetq_moe_route(p, 4, 9, 8, p, p, p, p, p, n) == ERR_INVALID
    assert lib.eetq_moe_route(p, 4, 0, 8, p, p, p, p, p, n) == ERR_INVALID
    assert lib.eetq_moe_route(p, 0, 2, 8, p, p, p, p, p, n) == ERR_INVALID
    assert lib.eetq_moe_route(p, 4, 2, 8, p, p, n, p, p, n) == ERR_INVALID
    # grouped GEMM: null pointers (sorted_slot only matters when gathering), layout shapes, E / k, flags, alignment
    ok = (p, p, p, p, p, p, p, 4, 2, 8, 256, 512, 1, 1, n)
    assert lib.eetq_w8a16_moe_gemm(n, *ok[1:]) == ERR_INVALID
    assert lib.eetq_w8a16_moe_gemm(p, p, p, p, n, p, p, 4, 2, 8, 256, 512, 1, 1, n) == ERR_INVALID
    assert lib.eetq_w8a16_moe_gemm(p, p, p, p, p, p, p, 4, 2, 8, 200, 512, 1, 1, n) == ERR_INVALID  # N % 16
    assert lib.eetq_w8a16_moe_gemm(p, p, p, p, p, p, p, 4, 2, 8, 256, 500, 1, 1, n) == ERR_INVALID  # K % 64
    assert lib.eetq_w8a16_moe_gemm(p, p, p, p, p, p, p, 4, 2, 2000, 256, 512, 1, 1, n) == ERR_INVALID
    assert lib.eetq_w8a16_moe_gemm(p, p, p, p, p, p, p, 4, 9, 8, 256, 512, 1, 1, n) == ERR_INVALID
    assert lib.eetq_w8a16_moe_gemm(p, p, p, p, p, p, p, 4, 2, 8, 256, 512, 2, 1, n) == ERR_INVALID
    assert lib.eetq_w8a16_moe_gemm(p, p, p, p, p, p, p, 4, 2, 8, 256, 512, 1, 3, n) == ERR_INVALID
    assert lib.eetq_w8a16_moe_gemm(ctypes.c_void_p(18), p, p, p, p, p, p, 4, 2, 8, 256, 512, 1, 1, n) == ERR_INVALID
    # combine: null pointer, weight dtype, H % 8, alignment
    assert lib.eetq_moe_combine_f16(n, p, p, 1, p, 4, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_f16(p, p, p, 2, p, 4, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_f16(p, p, p, 1, p, 4, 2, 100, n) == ERR_INVALID
    assert lib.eetq_moe_combine_f16(p, p, p, 1, ctypes.c_void_p(24), 4, 2, 256, n) == ERR_INVALID


def test_ctypes_binding_refuses_the_moe_layer():
    from eetq_amd import ops_ctypes
    with pytest.raises(RuntimeError, match="compiled EETQ module"):
        ops_ctypes.w8_a16_moe(None, None, None, None, None, None, None)


def _mixtral(experts=8, k=2, H=128, I=192):
    from transformers import MixtralConfig, MixtralForCausalLM
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=experts, num_experts_per_tok=k, vocab_size=256)
    return MixtralForCausalLM(cfg).half()


def _qwen3_moe():
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    cfg = Qwen3MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=64, num_hidden_layers=2,
                         num_attention_heads=4, num_key_value_heads=2, num_experts=16, num_experts_per_tok=4, vocab_size=256,
                         decoder_sparse_step=1, mlp_only_layers=[])
    return Qwen3MoeForCausalLM(cfg).half()


@pytest.mark.parametrize("make,E,H,I", [(_mixtral, 8, 128, 192), (_qwen3_moe, 16, 128, 64)])
def test_eet_quantize_experts_init_only(make, E, H, I):
    from eetq_amd.modules.qlinear import W8A16Experts, W8A16Linear
    from eetq_amd.utils.quantizer import eet_quantize
    model = make()
    eet_quantize(model, init_only=True, experts=True)
    layers = model.model.layers
    assert len(layers) == 2
    for layer in layers:
        ex = layer.mlp.experts
        assert isinstance(ex, W8A16Experts)
        assert (ex.gate_up_qweight.shape, ex.gate_up_qweight.dtype) == ((E, H, 2 * I), torch.int8)
        assert (ex.gate_up_scales.shape, ex.gate_up_scales.dtype) == ((E, 2 * I), torch.float16)
        assert (ex.down_qweight.shape, ex.down_qweight.dtype) == ((E, I, H), torch.int8)
        assert (ex.down_scales.shape, ex.down_scales.dtype) == ((E, H), torch.float16)
        assert isinstance(layer.self_attn.q_proj, W8A16Linear)
        assert not any(isinstance(m, torch.nn.Linear) for m in layer.mlp.modules())  # the routers are bare parameters


def test_eet_quantize_leaves_experts_alone_by_default():
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd.modules.qlinear import W8A16Linear
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()
    before = {n: p.clone() for n, p in model.named_parameters() if "experts" in n}
    eet_quantize(model, init_only=True)
    for layer in model.model.layers:
        assert type(layer.mlp.experts) is MixtralExperts
        assert isinstance(layer.self_attn.o_proj, W8A16Linear)
    after = dict(model.named_parameters())
    assert before and all(torch.equal(after[n], t) for n, t in before.items())


def _experts_module(**overrides):
    model = _mixtral()
    mod = model.model.layers[0].mlp.experts
    for k, v in overrides.items():
        setattr(mod, k, v)
    return mod


@pytest.mark.parametrize("overrides", [{"is_transposed": True}, {"has_bias": True}, {"act_fn": torch.nn.GELU()},
                                       {"has_gate": False}, {"is_concatenated": False}])
def test_from_experts_rejects_unsupported_forms(overrides):
    from eetq_amd.modules.qlinear import W8A16Experts
    with pytest.raises(ValueError):
        W8A16Experts.from_experts(_experts_module(**overrides))
    with pytest.raises(ValueError):
        W8A16Experts.from_experts(_experts_module(**overrides), init_only=True)


def test_from_experts_rejects_shapes_the_layout_cannot_take():
    from eetq_amd.modules.qlinear import W8A16Experts
    model = _mixtral(I=96)  # I % 64 != 0
    with pytest.raises(ValueError, match="I % 64"):
        W8A16Experts.from_experts(model.model.layers[0].mlp.experts)


def test_eet_quantize_warns_once_and_keeps_unsupported_experts():
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()
    for layer in model.model.layers:
        layer.mlp.experts.act_fn = torch.nn.GELU()
    with pytest.warns(UserWarning, match="2 experts module") as rec:
        eet_quantize(model, init_only=True, experts=True)
    assert len([w for w in rec if "experts module" in str(w.message)]) == 1
    assert all(type(layer.mlp.experts) is MixtralExperts for layer in model.model.layers)


def test_eet_quantize_drops_each_fp16_experts_module_before_the_next(monkeypatch):
    """Quantising holds one fp16 experts module at a time: by the time the next one is converted, every module already
    replaced is gone (no list of the originals survives the loop)."""
    import gc
    import weakref

    from eetq_amd.modules.qlinear import W8A16Experts
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()
    seen, alive_at_call = [], []
    real = W8A16Experts.from_experts.__func__

    def spy(cls, module, init_only=False):
        gc.collect()
        alive_at_call.append(sum(r() is not None for r in seen))
        seen.append(weakref.ref(module))
        return real(cls, module, init_only=init_only)

    monkeypatch.setattr(W8A16Experts, "from_experts", classmethod(spy))
    eet_quantize(model, init_only=True, experts=True)
    gc.collect()
    assert alive_at_call == [0, 0] and all(r() is None for r in seen)
