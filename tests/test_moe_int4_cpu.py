"""W4A16 mixture-of-experts surface without a GPU: the two int4 C entries are declared, exported and refuse bad
arguments before any launch; eet_quantize(experts=True, expert_bits=4) swaps transformers' 3-D experts modules for W4A16Experts
(init_only: buffers only) at half the int8 bytes, keeps the int8 default, leaves shapes the int4 tiles cannot take in fp16 and
rejects bad expert_bits before touching the model; and the glu8 claim the quantisation rests on, on the oracle alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eetq_w4a16_moe_gemm", "eetq_expand_i4_to_i8", "eetq_w8a16_moe_gemm_tiled_supported")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_int4_moe_entries_declared_and_exported(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr
    assert lib.eetq_abi_version() == 7
    assert "moe_int4.hip" in open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()


def test_int4_moe_gemm_rejects_bad_arguments_without_a_device(lib):
    p = ctypes.c_void_p(16)  # never dereferenced: every case fails its argument check first
    n = None
    f = lib.eetq_w4a16_moe_gemm
    ok = (p, p, p, p, p, p, p, 4, 2, 8, 256, 512, 1, 1, n)
    for i in (0, 1, 2, 3, 5, 6):  # x, w_packed, scales, offsets, active, y
        args = list(ok)
        args[i] = n
        assert f(*args) == ERR_INVALID, i
    assert f(p, p, p, p, n, p, p, 4, 2, 8, 256, 512, 1, 1, n) == ERR_INVALID  # sorted_slot matters when gathering
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 200, 512, 1, 1, n) == ERR_INVALID  # N % 16
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 256, 500, 1, 1, n) == ERR_INVALID  # K % 64
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 256, 448, 1, 1, n) == ERR_INVALID  # K % 64 == 0 but K % 128 != 0: int4 tiles are 128 deep
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 256, 64, 1, 1, n) == ERR_INVALID
    assert f(p, p, p, p, p, p, p, 4, 2, 2000, 256, 512, 1, 1, n) == ERR_INVALID
    assert f(p, p, p, p, p, p, p, 4, 2, 0, 256, 512, 1, 1, n) == ERR_INVALID
    assert f(p, p, p, p, p, p, p, 4, 9, 8, 256, 512, 1, 1, n) == ERR_INVALID
    assert f(p, p, p, p, p, p, p, 4, 0, 8, 256, 512, 1, 1, n) == ERR_INVALID
    assert f(p, p, p, p, p, p, p, 0, 2, 8, 256, 512, 1, 1, n) == ERR_INVALID
    # K = 512 passes the depth check (the call gets as far as the flag check behind it); K = 448 does not
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 256, 512, 2, 1, n) == ERR_INVALID
    assert b"gather and glu8" in lib.eetq_last_error()
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 256, 448, 2, 1, n) == ERR_INVALID
    assert b"K % 128" in lib.eetq_last_error()
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 256, 512, 1, 3, n) == ERR_INVALID
    assert f(p, p, p, p, p, p, p, 4, 2, 8, 256, 512, -1, 0, n) == ERR_INVALID
    m = ctypes.c_void_p(24)
    assert f(m, p, p, p, p, p, p, 4, 2, 8, 256, 512, 1, 1, n) == ERR_INVALID
    assert b"16-byte" in lib.eetq_last_error()
    assert f(p, m, p, p, p, p, p, 4, 2, 8, 256, 512, 1, 1, n) == ERR_INVALID
    assert f(p, p, p, p, p, p, m, 4, 2, 8, 256, 512, 1, 1, n) == ERR_INVALID


def test_expand_entry_rejects_bad_arguments_without_a_device(lib):
    f = lib.eetq_expand_i4_to_i8
    a, b, n = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 22), None
    assert f(n, b, 4096, n) == ERR_INVALID
    assert f(a, n, 4096, n) == ERR_INVALID
    assert f(a, b, 0, n) == ERR_INVALID
    assert f(a, b, 1000, n) == ERR_INVALID          # not whole 1 KiB tiles
    assert f(ctypes.c_void_p((1 << 20) + 8), b, 4096, n) == ERR_INVALID
    assert f(a, ctypes.c_void_p((1 << 22) + 8), 4096, n) == ERR_INVALID
    assert f(a, a, 4096, n) == ERR_INVALID          # in place
    assert f(a, ctypes.c_void_p((1 << 20) + 2048), 4096, n) == ERR_INVALID   # dst starts inside src
    assert f(ctypes.c_void_p((1 << 20) + 4096), a, 4096, n) == ERR_INVALID   # src starts inside dst's 2 * bytes_src


def test_tiled_support_query_is_the_tiled_entrys_shape_limits(lib):
    """eetq_w8a16_moe_gemm_tiled_supported: what the int4 layer's shape rule asks before it expands anything (host arithmetic)"""
    f = lib.eetq_w8a16_moe_gemm_tiled_supported
    assert f(512, 2, 8, 768, 512, 1) == 1 and f(512, 2, 8, 512, 384, 0) == 1
    assert f(512, 2, 8, 768, 256, 1) == 0          # K = 256 < 320: below the ring minimum
    assert f(512, 2, 8, 768, 320, 1) == 1
    assert f(512, 2, 8, 65536, 32768, 1) == 0      # N K = 2^31 per expert
    assert f(1 << 20, 2, 8, 768, 1024, 1) == 0     # 2^20 rows x 1024 x 2 bytes = 2 GiB of activations
    assert f(1 << 19, 2, 8, 768, 1024, 1) == 1 and f(1 << 19, 2, 8, 768, 1024, 0) == 0   # contiguous: T k rows
    assert f(0, 2, 8, 768, 512, 1) == 0 and f(4, 0, 8, 768, 512, 1) == 0


def test_ctypes_binding_refuses_the_int4_moe_layer():
    from eetq_amd import ops_ctypes
    with pytest.raises(RuntimeError, match="compiled EETQ module"):
        ops_ctypes.w4_a16_moe(None, None, None, None, None, None, None)


def test_exports():
    import eetq
    import eetq_amd
    import eetq_amd.modules
    from eetq_amd import ops
    from eetq_amd.modules.qlinear import W4A16Experts
    assert eetq_amd.W4A16Experts is W4A16Experts and eetq_amd.modules.W4A16Experts is W4A16Experts
    assert eetq.W4A16Experts is W4A16Experts
    assert "w4_a16_moe" in ops.__all__ and callable(ops.w4_a16_moe)


def _mixtral(experts=8, k=2, H=128, I=256):
    from transformers import MixtralConfig, MixtralForCausalLM
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=experts, num_experts_per_tok=k, vocab_size=256)
    return MixtralForCausalLM(cfg).half()


def _qwen3_moe():
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    cfg = Qwen3MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=128, num_hidden_layers=2,
                         num_attention_heads=4, num_key_value_heads=2, num_experts=16, num_experts_per_tok=4, vocab_size=256,
                         decoder_sparse_step=1, mlp_only_layers=[])
    return Qwen3MoeForCausalLM(cfg).half()


def _buffer_bytes(mod):
    return sum(b.numel() * b.element_size() for n, b in mod.named_buffers() if n.endswith("qweight"))


@pytest.mark.parametrize("make,E,H,I", [(_mixtral, 8, 128, 256), (_qwen3_moe, 16, 128, 128)])
def test_eet_quantize_expert_bits_4_init_only(make, E, H, I):
    from eetq_amd.modules.qlinear import W4A16Experts, W8A16Experts, W8A16Linear
    from eetq_amd.utils.quantizer import eet_quantize, set_trainable
    model, model8, model_default = make(), make(), make()
    eet_quantize(model, init_only=True, experts=True, expert_bits=4)
    eet_quantize(model8, init_only=True, experts=True, expert_bits=8)
    eet_quantize(model_default, init_only=True, experts=True)
    assert len(model.model.layers) == 2
    for layer, layer8, layer_d in zip(model.model.layers, model8.model.layers, model_default.model.layers):
        ex = layer.mlp.experts
        assert type(ex) is W4A16Experts
        assert (ex.gate_up_qweight.shape, ex.gate_up_qweight.dtype) == ((E, H, I), torch.int8)
        assert (ex.gate_up_scales.shape, ex.gate_up_scales.dtype) == ((E, 2 * I), torch.float16)
        assert (ex.down_qweight.shape, ex.down_qweight.dtype) == ((E, I, H // 2), torch.int8)
        assert (ex.down_scales.shape, ex.down_scales.dtype) == ((E, H), torch.float16)
        assert set(ex.state_dict()) == {"gate_up_qweight", "gate_up_scales", "down_qweight", "down_scales"}
        assert "bits=4" in ex.extra_repr()
        assert type(layer8.mlp.experts) is W8A16Experts and type(layer_d.mlp.experts) is W8A16Experts
        assert 2 * _buffer_bytes(ex) == _buffer_bytes(layer8.mlp.experts)
        assert isinstance(layer.self_attn.q_proj, W8A16Linear)   # the nn.Linear pass is unchanged
    # set_trainable passes the int4 experts by
    n = set_trainable(model, True)
    assert n == sum(isinstance(m, W8A16Linear) for m in model.modules())
    assert not any(getattr(m, "trainable", False) for m in model.modules() if isinstance(m, W4A16Experts))


def test_expert_bits_4_leaves_shapes_the_int4_tiles_cannot_take_in_fp16():
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd.modules.qlinear import W4A16Experts, W8A16Experts
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral(I=192)   # I % 64 == 0 (int8 takes it) but I % 128 != 0
    assert W8A16Experts.unsupported_reason(model.model.layers[0].mlp.experts) is None
    assert "128" in W4A16Experts.unsupported_reason(model.model.layers[0].mlp.experts)
    with pytest.raises(ValueError, match="I % 128"):
        W4A16Experts.from_experts(model.model.layers[0].mlp.experts, init_only=True)
    with pytest.warns(UserWarning, match="2 experts module") as rec:
        eet_quantize(model, init_only=True, experts=True, expert_bits=4)
    msgs = [str(w.message) for w in rec if "experts module" in str(w.message)]
    assert len(msgs) == 1 and "layers.0.mlp.experts" in msgs[0] and "layers.1.mlp.experts" in msgs[0] and "I = 192" in msgs[0]
    assert all(type(layer.mlp.experts) is MixtralExperts for layer in model.model.layers)


@pytest.mark.parametrize("kwargs", [{"expert_bits": 3}, {"expert_bits": 16}, {"expert_bits": "4"},
                                    {"expert_bits": 4, "trainable": True}, {"expert_bits": 4, "experts": False}])
def test_bad_expert_bits_raise_before_the_model_is_touched(kwargs):
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()
    before = [(n, type(m), id(m)) for n, m in model.named_modules()]
    with pytest.raises(ValueError, match="expert_bits"):
        eet_quantize(model, init_only=True, **dict({"experts": True}, **kwargs))
    assert [(n, type(m), id(m)) for n, m in model.named_modules()] == before


@pytest.mark.parametrize("overrides", [{"is_transposed": True}, {"has_bias": True}, {"act_fn": torch.nn.GELU()},
                                       {"has_gate": False}, {"is_concatenated": False}])
def test_from_experts_rejects_unsupported_forms(overrides):
    from eetq_amd.modules.qlinear import W4A16Experts
    mod = _mixtral().model.layers[0].mlp.experts
    for k, v in overrides.items():
        setattr(mod, k, v)
    with pytest.raises(ValueError):
        W4A16Experts.from_experts(mod, init_only=True)


def test_glu8_permutation_commutes_with_int4_quantisation_on_the_oracle():
    """per-channel quantisation commutes with a permutation of the output channels: quantising the glu8-permuted fp16 matrix gives
    the glu8 permutation of the unpermuted matrix's integers and scales, bit for bit -- what W4A16Experts.from_experts relies on"""
    import oracle
    from eetq_amd.utils.fuse import _glu8_interleave_columns
    H, I = 128, 256
    rng = np.random.default_rng(4)
    w = (rng.standard_normal((H, 2 * I)) * 0.05).astype(np.float16)
    wt = torch.from_numpy(w)
    perm_w = _glu8_interleave_columns(wt[:, :I], wt[:, I:]).contiguous().numpy()
    q, s = oracle.quantize_i4(w)
    qp, sp = oracle.quantize_i4(perm_w)
    vals, vals_p = oracle.i4_values(q), oracle.i4_values(qp)
    assert vals.min() == -8 and vals.max() == 7
    vt, st = torch.from_numpy(vals), torch.from_numpy(s)
    assert np.array_equal(vals_p, _glu8_interleave_columns(vt[:, :I], vt[:, I:]).numpy())
    assert sp.tobytes() == _glu8_interleave_columns(st[:I], st[I:]).contiguous().numpy().tobytes()
    # the permutation is a real one: tile 0 = gate columns 0..7 then up columns 0..7
    assert np.array_equal(perm_w[:, :8], w[:, :8]) and np.array_equal(perm_w[:, 8:16], w[:, I:I + 8])
    assert not np.array_equal(vals_p, vals)
