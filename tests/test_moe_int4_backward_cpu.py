"""Training through the int4 experts, the part that needs no GPU: eetq_w4a16_moe_gemm_t is declared, exported and
refuses bad arguments before any launch, naming itself; the two operators are listed by both bindings; the public switch
(set_trainable(..., int4_experts=True), W4A16Experts.trainable, eet_quantize's refusal); and the machine code of the grouped int4
instantiation, alone in its object."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "eetq_w4a16_moe_gemm_t"
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


# ---- 1. ABI surface -----------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_typed(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    assert re.search(r"\bint\s+eetq_w4a16_moe_gemm_t\s*\(const void\* dy, const int8_t\* w_packed_i4, const void\* scales, "
                     r"const int\* offsets, const int\* active,\s*void\* dx, int T, int k, int E, int N, int K, void\* stream\);", hdr)
    assert ENTRY in _lib.EXPORTED_SYMBOLS
    assert lib.eetq_w4a16_moe_gemm_t.argtypes == lib.eetq_w8a16_moe_gemm_t.argtypes   # the int8 entry's argument order
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr
    assert lib.eetq_abi_version() == 7
    assert "moe_gemm_t_int4.hip" in open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()


# ---- 2. refusals before any launch --------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_without_a_device(lib):
    f = lib.eetq_w4a16_moe_gemm_t
    p, m, n = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8), None   # never dereferenced: every case fails a check
    ok = [p, p, p, p, p, p, 4, 2, 8, 256, 512, n]                              # dy, w, scales, offsets, active, dx, T, k, E, N, K

    def refused(what, **change):
        args = list(ok)
        for i, v in change.items():
            args[int(i[1:])] = v
        assert f(*args) == ERR_INVALID, what
        msg = lib.eetq_last_error()
        assert ENTRY.encode() in msg, (what, msg)
        return msg
    for i in range(6):
        assert b"null pointer" in refused("null %d" % i, **{"a%d" % i: n})
    for E in (0, -1, 1025):
        assert b"E must be" in refused("E", a8=E)
    for k in (0, 9, -2):
        assert b"k must be" in refused("k", a7=k)
    assert b"T must be" in refused("T = 0", a6=0)
    assert b"T must be" in refused("T < 0", a6=-3)
    assert b"T must be" in refused("T k > 2^30", a6=(1 << 29) + 1)
    assert b"K % 128" in refused("K % 128", a10=448)                            # 64-deep: an int8 depth, not an int4 one
    assert b"K % 128" in refused("K = 64", a10=64)
    assert b"K % 128" in refused("K = 0", a10=0)
    assert b"N % 16" in refused("N % 16", a9=200)
    assert b"N % 16" in refused("N = 0", a9=0)
    # index arithmetic: T k max(N, K) < 2^40 and E K N / 2 bytes < 2^40 (which keep the grid below 2^31)
    assert b"too large" in refused("gradient", a6=1 << 29, a9=1 << 20)
    assert b"too large" in refused("stack", a8=1024, a9=1 << 20, a10=1 << 21)
    for i in (0, 1, 5):                                                         # dy, weight, dx
        assert b"16-byte" in refused("alignment %d" % i, **{"a%d" % i: m})


# ---- 3. operator lists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["ops", "ops_ctypes"])
def test_operators_are_listed(binding):
    mod = importlib.import_module("eetq_amd." + binding)
    for name in ("w4_a16_moe_train", "w4_a16_moe_backward"):
        assert name in mod.__all__ and callable(getattr(mod, name))


def test_ctypes_binding_refuses_and_names_the_compiled_module():
    from eetq_amd import ops_ctypes
    with pytest.raises(RuntimeError, match="w4_a16_moe_train needs the compiled EETQ module"):
        ops_ctypes.w4_a16_moe_train(None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="w4_a16_moe_backward needs the compiled EETQ module"):
        ops_ctypes.w4_a16_moe_backward(None, None, None, None, None, None, None, None, None)


def test_compiled_operators_reject_cpu_tensors():
    from eetq_amd import _ext
    ops = _ext.load()   # the compiled module itself, whichever binding eetq_amd.ops has picked
    E, H, I, T, k = 2, 128, 128, 3, 2
    x = torch.zeros(T, H, dtype=torch.float16)
    idx, wts = torch.zeros(T, k, dtype=torch.long), torch.ones(T, k)
    stacks = (torch.zeros(E, H, I, dtype=torch.int8), torch.ones(E, 2 * I, dtype=torch.float16),
              torch.zeros(E, I, H // 2, dtype=torch.int8), torch.ones(E, H, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="w4_a16_moe_train: hidden must be a float16 GPU tensor"):
        ops.w4_a16_moe_train(x, idx, wts, *stacks)
    with pytest.raises(RuntimeError, match="w4_a16_moe_train: hidden must be a float16 GPU tensor"):
        ops.w4_a16_moe_train(hidden=x, top_k_index=idx, top_k_weights=wts, gate_up_qweight=stacks[0], gate_up_scales=stacks[1],
                             down_qweight=stacks[2], down_scales=stacks[3], path="decode")
    tables = torch.zeros(2 * E + 1 + 2 * T * k + min(E, T * k), dtype=torch.int32)
    gate_up, y = torch.zeros(T * k, 2 * I, dtype=torch.float16), torch.zeros(T * k, H, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="w4_a16_moe_backward: grad_out must be a float16 GPU tensor"):
        ops.w4_a16_moe_backward(x, wts, tables, gate_up, y, *stacks, need_input_grad=True, need_weights_grad=False)


# ---- 4. the switch ------------------------------------------------------------------------------------------------------------
def _mixtral():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.MixtralConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                                     num_key_value_heads=2, num_local_experts=8, num_experts_per_tok=2, vocab_size=256)
    return transformers.MixtralForCausalLM(cfg).half()


def test_trainable_is_a_class_attribute_and_the_switch_needs_its_keyword():
    from eetq_amd.modules.qlinear import W4A16Experts, W4A16MoeFunction
    from eetq_amd.utils.quantizer import eet_quantize, set_trainable
    assert W4A16Experts.trainable is False
    assert issubclass(W4A16MoeFunction, torch.autograd.Function)
    model = _mixtral()
    eet_quantize(model, init_only=True, experts=True, expert_bits=4)
    experts = [m for m in model.modules() if isinstance(m, W4A16Experts)]
    assert len(experts) == 2 and all(m.trainable is False for m in experts)
    keys = set(experts[0].state_dict())
    assert keys == {"gate_up_qweight", "gate_up_scales", "down_qweight", "down_scales"}
    without = set_trainable(model, True)                       # the two-argument call: int4 experts passed by, not counted
    assert without > 0 and all(m.trainable is False for m in experts)
    assert set_trainable(model, True, int4_experts=True) == without + 2
    assert all(m.trainable is True for m in experts)
    assert set(experts[0].state_dict()) == keys and "trainable" not in experts[0].state_dict()
    assert set_trainable(model, False) == without and all(m.trainable is True for m in experts)
    assert set_trainable(model, False, int4_experts=True) == without + 2
    assert all(m.trainable is False for m in experts)


def test_eet_quantize_still_refuses_and_says_how():
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral()
    before = {n: type(m).__name__ for n, m in model.named_modules()}
    with pytest.raises(ValueError, match="expert_bits") as err:
        eet_quantize(model, init_only=True, experts=True, expert_bits=4, trainable=True)
    assert "int4_experts" in str(err.value) and "set_trainable" in str(err.value)
    assert {n: type(m).__name__ for n, m in model.named_modules()} == before


@pytest.mark.parametrize("kind", ["mixtral", "glm4_moe"])
def test_trainable_int4_experts_keep_the_block_unfused_in_grad_mode(kind):
    """softmax (Mixtral) and sigmoid (GLM-4-MoE) blocks alike: with nothing else asking for the unfused route (frozen router, input
    without grad, no hooks), the block op serves the call until the int4 experts are trainable in grad mode"""
    from eetq_amd.modules.qlinear import EetqSparseMoeBlock, W4A16Experts
    from eetq_amd.utils.quantizer import eet_quantize, set_trainable
    from test_moe_router_sigmoid_cpu import tiny
    torch.manual_seed(0)
    model = _mixtral() if kind == "mixtral" else tiny(kind).half()
    eet_quantize(model, init_only=True, experts=True, expert_bits=4, router=True)
    blocks = [m for m in model.modules() if isinstance(m, EetqSparseMoeBlock)]
    assert len(blocks) == 2 and all(isinstance(b.experts, W4A16Experts) for b in blocks)
    assert blocks[0].gate.is_sigmoid == (kind != "mixtral")
    for prm in model.parameters():
        prm.requires_grad_(False)
    h = torch.zeros(1, 3, 128, dtype=torch.float16)
    assert all(b.fused(h) for b in blocks)
    set_trainable(model, True)                                  # without the keyword nothing changes for the int4 blocks
    assert all(b.fused(h) for b in blocks)
    set_trainable(model, True, int4_experts=True)
    assert not any(b.fused(h) for b in blocks)
    with torch.no_grad():
        assert all(b.fused(h) for b in blocks)
    set_trainable(model, False, int4_experts=True)
    assert all(b.fused(h) for b in blocks)


# ---- 5. the new object --------------------------------------------------------------------------------------------------------
def test_grouped_int4_kernel_machine_code(tmp_path):
    """The grouped int4 instantiation alone in its object: transposed LDS reads feeding 32x32x16 MFMAs, no scratch, no spills, and
    few enough registers for the two workgroups per CU its launch bounds ask for."""
    from eetq_amd import _lib
    _lib.lib()   # builds the library (and with it moe_gemm_t_int4.o) when the sources are newer
    llvm = "/opt/rocm/lib/llvm/bin"
    objdump = os.path.join(llvm, "llvm-objdump") if os.path.exists(os.path.join(llvm, "llvm-objdump")) else shutil.which("llvm-objdump")
    readelf = os.path.join(llvm, "llvm-readelf") if os.path.exists(os.path.join(llvm, "llvm-readelf")) else shutil.which("llvm-readelf")
    assert objdump and readelf, "llvm-objdump / llvm-readelf not found"
    local = os.path.join(str(tmp_path), "moe_gemm_t_int4.o")
    shutil.copy(os.path.join(ROOT, "eetq_amd", "csrc", "moe_gemm_t_int4.o"), local)
    subprocess.run([objdump, "--offloading", local], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    dev = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(str(tmp_path))
    dev = os.path.join(str(tmp_path), dev[0])
    text = subprocess.run([objdump, "-d", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    syms = re.findall(r"<(_Z\w*gemm_t_kernel\w*)>:", text)
    assert len(syms) == 1 and "ILb1ELi4E" in syms[0], syms              # grouped map, BITS = 4
    assert re.search(r"\bds_read_b64_tr_b16\b", text)
    assert re.search(r"\bv_mfma_f32_32x32x16_f16\b", text)
    notes = subprocess.run([readelf, "--notes", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    meta = [k for k in re.split(r"\n\s*- \.", notes) if "gemm_t_kernel" in k]
    assert len(meta) == 1
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta[0])
    assert re.search(r"\.vgpr_spill_count:\s+0\b", meta[0])
    assert re.search(r"\.sgpr_spill_count:\s+0\b", meta[0])
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", meta[0]).group(1)) <= 256
