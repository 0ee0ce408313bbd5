"""The int4 input gradient (eetq_w4a16_gemm_t, w4_a16_gemm_t, W4A16Linear.trainable, eet_quantize(bits=4)) without a GPU: the
quantiser's choice of module per layer, its warning and refusals, the trainable flag, the ABI tables and the operator lists."""
import os
import re
import warnings

import pytest
import torch
import torch.nn as nn

from conftest import ROOT


def _tiny_llama():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=4, vocab_size=1000, max_position_embeddings=256)
    torch.manual_seed(0)
    return transformers.LlamaForCausalLM(cfg).half().eval()


def _types(model):
    return {n: type(m).__name__ for n, m in model.named_modules()}


def test_bits4_builds_w4a16_linear_for_every_projection():
    from eetq_amd.modules.qlinear import W4A16Linear
    from eetq_amd.utils.quantizer import eet_quantize
    model = _tiny_llama()
    shapes = {n: (m.in_features, m.out_features) for n, m in model.named_modules() if isinstance(m, nn.Linear)}
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # every shape fits: no warning
        eet_quantize(model, init_only=True, bits=4)
    assert len(shapes) == 2 * 7 + 1
    for name, (k, n) in shapes.items():
        mod = model.get_submodule(name)
        if name == "lm_head":
            assert type(mod) is nn.Linear
            continue
        assert type(mod) is W4A16Linear, name
        assert mod.qweight.shape == (k, n // 2) and mod.qweight.dtype == torch.int8
        assert mod.weight_scales.shape == (n,) and mod.weight_scales.dtype == torch.float16
        assert mod.trainable is False


class _Odd(nn.Module):
    def __init__(self):
        super().__init__()
        self.fits = nn.Linear(128, 32, bias=False).half()
        self.odd = nn.Linear(192, 64, bias=False).half()                 # 192 % 128 != 0: stays int8


def test_bits4_leaves_other_shapes_on_int8_with_one_warning():
    from eetq_amd.modules.qlinear import W4A16Linear, W8A16Linear
    from eetq_amd.utils.quantizer import eet_quantize
    model = _Odd()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        eet_quantize(model, init_only=True, bits=4)
    assert type(model.fits) is W4A16Linear
    assert type(model.odd) is W8A16Linear and model.odd.qweight.shape == (192, 64)
    mine = [w for w in seen if issubclass(w.category, UserWarning) and "eet_quantize" in str(w.message)]
    assert len(mine) == 1
    assert "odd" in str(mine[0].message) and "fits" not in str(mine[0].message)


def test_default_bits_is_8_and_changes_nothing():
    from eetq_amd.modules.qlinear import W8A16Linear
    from eetq_amd.utils.quantizer import eet_quantize
    model = _Odd()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        eet_quantize(model, init_only=True)
    assert type(model.fits) is W8A16Linear and type(model.odd) is W8A16Linear


@pytest.mark.parametrize("bits", [3, 16, "4"])
def test_other_bits_raise_before_the_model_is_touched(bits):
    from eetq_amd.utils.quantizer import eet_quantize
    model = _Odd()
    before = _types(model)
    with pytest.raises(ValueError, match="bits must be 8 or 4"):
        eet_quantize(model, init_only=True, bits=bits)
    assert _types(model) == before


def test_bits4_trainable_sets_every_w4a16_linear():
    from eetq_amd.modules.qlinear import W4A16Linear
    from eetq_amd.utils.quantizer import eet_quantize, set_trainable
    model = _tiny_llama()
    eet_quantize(model, init_only=True, bits=4, trainable=True)
    mods = [m for m in model.modules() if isinstance(m, W4A16Linear)]
    assert len(mods) == 14 and all(m.trainable is True for m in mods)
    assert set_trainable(model, False) == 14
    assert all(m.trainable is False for m in mods)
    assert set_trainable(model, True) == 14


def test_trainable_is_a_class_attribute_not_state():
    from eetq_amd.modules.qlinear import W4A16Linear
    assert W4A16Linear.trainable is False
    mod = W4A16Linear(128, 32, bias=True, dev="cpu")
    assert mod.trainable is False
    keys = set(mod.state_dict())
    mod.trainable = True
    assert set(mod.state_dict()) == keys == {"qweight", "weight_scales", "bias"}
    assert "trainable" not in mod.state_dict()


def test_entry_point_is_declared_and_registered():
    from eetq_amd import _lib
    text = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    assert re.search(r"\bint\s+eetq_w4a16_gemm_t\s*\(const void\* in, const void\* weight_i4, const void\* scale, void\* out, "
                     r"int M, int N, int K, void\* stream\);", text)
    assert "#define EETQ_AMD_ABI_VERSION 7" in text
    assert "eetq_w4a16_gemm_t" in _lib.EXPORTED_SYMBOLS
    lib = _lib.lib()
    assert lib.eetq_w4a16_gemm_t.argtypes == lib.eetq_w8a16_gemm_t.argtypes
    assert lib.eetq_abi_version() == 7


def test_argument_validation_without_gpu():
    import ctypes

    from eetq_amd import _lib
    lib = _lib.lib()
    assert lib.eetq_w4a16_gemm_t(None, None, None, None, 1, 64, 128, None) == -1
    assert b"null pointer" in lib.eetq_last_error()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.eetq_w4a16_gemm_t(p, p, p, p, 1, 64, 192, None) == -1     # K % 128
    assert b"multiple of 128" in lib.eetq_last_error()
    assert lib.eetq_w4a16_gemm_t(p, p, p, p, 1, 24, 128, None) == -1     # N % 16
    assert b"multiple of 16" in lib.eetq_last_error()
    assert lib.eetq_w4a16_gemm_t(p, p, p, p, 0, 64, 128, None) == -1     # M < 1
    assert b"invalid GEMM shape" in lib.eetq_last_error()


@pytest.mark.parametrize("binding", ["ops", "ops_ctypes"])
def test_operator_is_listed_and_rejects_cpu_tensors(binding):
    import importlib
    mod = importlib.import_module("eetq_amd." + binding)
    assert "w4_a16_gemm_t" in mod.__all__
    g = torch.zeros(2, 64, dtype=torch.float16)
    w = torch.zeros(128, 32, dtype=torch.int8)
    s = torch.ones(64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        mod.w4_a16_gemm_t(g, w, s)


def test_int4_kernel_machine_code(tmp_path):
    """The int4 instantiation alone in its object: transposed LDS reads feeding 32x32x16 MFMAs, no scratch, no spills, and few
    enough registers for the two workgroups per CU its launch bounds ask for."""
    import shutil
    import subprocess

    from eetq_amd import _lib
    _lib.lib()   # builds the library (and with it gemm_t_int4.o) when the sources are newer
    llvm = "/opt/rocm/lib/llvm/bin"
    objdump = os.path.join(llvm, "llvm-objdump") if os.path.exists(os.path.join(llvm, "llvm-objdump")) else shutil.which("llvm-objdump")
    readelf = os.path.join(llvm, "llvm-readelf") if os.path.exists(os.path.join(llvm, "llvm-readelf")) else shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf not found"
    local = os.path.join(str(tmp_path), "gemm_t_int4.o")
    shutil.copy(os.path.join(ROOT, "eetq_amd", "csrc", "gemm_t_int4.o"), local)
    subprocess.run([objdump, "--offloading", local], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    dev = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(str(tmp_path))
    dev = os.path.join(str(tmp_path), dev[0])
    text = subprocess.run([objdump, "-d", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    syms = re.findall(r"<(_Z\w*gemm_t_kernel\w*)>:", text)
    assert len(syms) == 1 and "ILb0ELi4E" in syms[0], syms              # plain map, BITS = 4; no grouped int4 form
    assert re.search(r"\bds_read_b64_tr_b16\b", text)
    assert re.search(r"\bv_mfma_f32_32x32x16_f16\b", text)
    notes = subprocess.run([readelf, "--notes", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    meta = [k for k in re.split(r"\n\s*- \.", notes) if "gemm_t_kernel" in k]
    assert len(meta) == 1
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[0])
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[0])
    assert re.search(r"\.sgpr_spill_count:\s+0\b", meta[0])
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta[0]).group(1)) <= 256
