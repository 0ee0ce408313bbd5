"""The routed-experts backward without a GPU: the three C entries are declared, exported and prototyped within ABI
revision 7 and refuse bad arguments before any launch; the ctypes binding refuses both ops; set_trainable and
eet_quantize(trainable=True) set the opt-in flag on every quantised module and the default leaves it off; the grouped input-gradient
kernel's machine code feeds transposed LDS reads into 32x32x16 MFMAs without scratch or spills."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eetq_w8a16_moe_gemm_t", "eetq_moe_combine_bwd_f16", "eetq_silu_mul_glu8_bwd_f16")
ERR_INVALID = -1
LLVM_BIN = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_entries_declared_exported_and_prototyped(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes, name   # _declare gave it a prototype
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr
    assert lib.eetq_abi_version() == 7


def test_grouped_gemm_t_rejects_bad_arguments(lib):
    p, n = ctypes.c_void_p(16), None
    ok = [p, p, p, p, p, p, 4, 2, 8, 256, 512, n]   # dy, w, s, offsets, active, dx, T, k, E, N, K, stream

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.eetq_w8a16_moe_gemm_t(*a)

    for i in range(6):                                       # every pointer
        assert call(**{"a%d" % i: n}) == ERR_INVALID, i
    assert call(a8=0) == ERR_INVALID and call(a8=1025) == ERR_INVALID         # E
    assert call(a7=0) == ERR_INVALID and call(a7=9) == ERR_INVALID            # k
    assert call(a6=0) == ERR_INVALID                                          # T
    assert call(a10=500) == ERR_INVALID and b"K % 64" in lib.eetq_last_error()
    assert call(a9=200) == ERR_INVALID and b"N % 16" in lib.eetq_last_error()
    for i in (0, 1, 5):                                      # dy, weight, dx alignment
        assert call(**{"a%d" % i: ctypes.c_void_p(24)}) == ERR_INVALID, i
        assert b"aligned" in lib.eetq_last_error()


def test_combine_bwd_rejects_bad_arguments(lib):
    p, n = ctypes.c_void_p(16), None
    # dout, y, position, weights, w_dtype, dy, dw, T, k, H, stream; dw may be null
    assert lib.eetq_moe_combine_bwd_f16(n, p, p, p, 1, p, p, 4, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_bwd_f16(p, n, p, p, 1, p, p, 4, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_bwd_f16(p, p, n, p, 1, p, p, 4, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_bwd_f16(p, p, p, n, 1, p, p, 4, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_bwd_f16(p, p, p, p, 1, n, p, 4, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_bwd_f16(p, p, p, p, 2, p, p, 4, 2, 256, n) == ERR_INVALID   # fp64 weights
    assert b"fp16 or fp32" in lib.eetq_last_error()
    assert lib.eetq_moe_combine_bwd_f16(p, p, p, p, 1, p, n, 4, 2, 100, n) == ERR_INVALID   # H % 8
    assert lib.eetq_moe_combine_bwd_f16(p, p, p, p, 1, p, n, 0, 2, 256, n) == ERR_INVALID
    assert lib.eetq_moe_combine_bwd_f16(p, p, p, p, 1, p, n, 4, 0, 256, n) == ERR_INVALID
    for i in (0, 1, 5):
        a = [p, p, p, p, 1, p, n, 4, 2, 256, n]
        a[i] = ctypes.c_void_p(24)
        assert lib.eetq_moe_combine_bwd_f16(*a) == ERR_INVALID, i


def test_silu_bwd_rejects_bad_arguments(lib):
    p, n = ctypes.c_void_p(16), None
    assert lib.eetq_silu_mul_glu8_bwd_f16(n, p, p, 4, 64, n) == ERR_INVALID
    assert lib.eetq_silu_mul_glu8_bwd_f16(p, n, p, 4, 64, n) == ERR_INVALID
    assert lib.eetq_silu_mul_glu8_bwd_f16(p, p, n, 4, 64, n) == ERR_INVALID
    assert lib.eetq_silu_mul_glu8_bwd_f16(p, p, p, 0, 64, n) == ERR_INVALID
    assert lib.eetq_silu_mul_glu8_bwd_f16(p, p, p, 4, 60, n) == ERR_INVALID
    for i in range(3):
        a = [p, p, p, 4, 64, n]
        a[i] = ctypes.c_void_p(24)
        assert lib.eetq_silu_mul_glu8_bwd_f16(*a) == ERR_INVALID, i


def test_ctypes_binding_refuses_the_training_ops():
    from eetq_amd import ops_ctypes
    assert {"w8_a16_moe_train", "w8_a16_moe_backward"} <= set(ops_ctypes.__all__)
    with pytest.raises(RuntimeError, match="compiled EETQ module"):
        ops_ctypes.w8_a16_moe_train(None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="compiled EETQ module"):
        ops_ctypes.w8_a16_moe_backward(None, None, None, None, None, None, None, None, None, True, True)


def _mixtral():
    from transformers import MixtralConfig, MixtralForCausalLM
    cfg = MixtralConfig(hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=8, num_experts_per_tok=2, vocab_size=256)
    return MixtralForCausalLM(cfg).half()


def _qwen3_moe():
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM
    cfg = Qwen3MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=64, num_hidden_layers=2,
                         num_attention_heads=4, num_key_value_heads=2, num_experts=16, num_experts_per_tok=4, vocab_size=256,
                         decoder_sparse_step=1, mlp_only_layers=[])
    return Qwen3MoeForCausalLM(cfg).half()


def _quantised(model):
    from eetq_amd.modules.qlinear import W8A16Experts, W8A16Linear
    return [m for m in model.modules() if isinstance(m, (W8A16Linear, W8A16Experts))]


@pytest.mark.parametrize("make", [_mixtral, _qwen3_moe])
def test_trainable_flag_is_opt_in(make):
    from eetq_amd.modules.qlinear import W8A16Experts
    from eetq_amd.utils import eet_quantize, set_trainable
    model = make()
    eet_quantize(model, init_only=True, experts=True)
    mods = _quantised(model)
    assert sum(isinstance(m, W8A16Experts) for m in mods) == 2
    assert mods and not any(m.trainable for m in mods)           # the default leaves every module inference-only
    assert set_trainable(model, True) == len(mods)
    assert all(m.trainable for m in mods)
    keys = {n for n, _ in model.named_buffers()} | {n for n, _ in model.named_parameters()}
    assert not any("trainable" in k for k in keys)                # a plain attribute, not a buffer: state dicts do not change
    assert set_trainable(model, False) == len(mods)
    assert not any(m.trainable for m in mods)

    model = make()
    eet_quantize(model, init_only=True, experts=True, trainable=True)
    mods = _quantised(model)
    assert sum(isinstance(m, W8A16Experts) for m in mods) == 2 and all(m.trainable for m in mods)
    assert {n for n, _ in model.named_buffers()} | {n for n, _ in model.named_parameters()} == keys


def _device_object(tmp_path):
    objdump = os.path.join(LLVM_BIN, "llvm-objdump")
    if not os.path.exists(objdump):
        objdump = shutil.which("llvm-objdump")
    assert objdump, "llvm-objdump not found"
    local = os.path.join(str(tmp_path), "gemm_t.o")
    shutil.copy(os.path.join(ROOT, "eetq_amd", "csrc", "gemm_t.o"), local)
    subprocess.run([objdump, "--offloading", local], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    dev = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(str(tmp_path))
    return objdump, os.path.join(str(tmp_path), dev[0])


def _grouped_symbol(text):
    # the grouped instantiation of the template kernel: gemm_t_kernel<true> (Itanium mangling ILb1E)
    syms = re.findall(r"<(_Z\w*gemm_t_kernelILb1E\w*)>:", text)
    assert len(syms) == 1, syms
    return syms[0]


def test_grouped_kernel_machine_code(lib, tmp_path):
    objdump, dev = _device_object(tmp_path)
    text = subprocess.run([objdump, "-d", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    sym = _grouped_symbol(text)
    body = text.split("<%s>:" % sym, 1)[1].split("\n\n", 1)[0]
    assert re.search(r"\bds_read_b64_tr_b16\b", body)
    assert re.search(r"\bv_mfma_f32_32x32x16_f16\b", body)
    readelf = os.path.join(LLVM_BIN, "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    notes = subprocess.run([readelf, "--notes", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    meta = [k for k in re.split(r"\n\s*- \.", notes) if sym in k]
    assert meta, "no code-object metadata for the grouped kernel"
    for k in meta:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", k), k
        assert re.search(r"\.vgpr_spill_count:\s+0\b", k), k
        assert re.search(r"\.sgpr_spill_count:\s+0\b", k), k
