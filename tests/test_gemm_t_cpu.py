"""eetq_w8a16_gemm_t (the projection's input gradient, ABI revision 7) without a GPU: the symbol and the revision, argument
validation before any HIP call, the machine code of the kernel (transposed LDS reads feeding 32x32x16 MFMAs, no scratch) and
the operator's refusal of CPU tensors in both bindings."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

OBJ = os.path.join(ROOT, "eetq_amd", "csrc", "gemm_t.o")
LLVM_BIN = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()   # builds the library (and with it gemm_t.o) when the sources are newer


def test_symbol_and_abi_revision(lib):
    from eetq_amd import _lib
    assert hasattr(lib, "eetq_w8a16_gemm_t")
    assert "eetq_w8a16_gemm_t" in _lib.EXPORTED_SYMBOLS
    assert lib.eetq_abi_version() == 7


def test_argument_validation_without_gpu(lib):
    assert lib.eetq_w8a16_gemm_t(None, None, None, None, 1, 64, 64, None) == -1
    assert b"null pointer" in lib.eetq_last_error()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.eetq_w8a16_gemm_t(p, p, p, p, 1, 64, 100, None) == -1     # K % 64
    assert b"multiple of 64" in lib.eetq_last_error()
    assert lib.eetq_w8a16_gemm_t(p, p, p, p, 1, 24, 64, None) == -1      # N % 16
    assert b"multiple of 16" in lib.eetq_last_error()
    assert lib.eetq_w8a16_gemm_t(p, p, p, p, 0, 64, 64, None) == -1      # M < 1
    assert b"invalid GEMM shape" in lib.eetq_last_error()


def _device_object(tmp_path):
    objdump = os.environ.get("LLVM_OBJDUMP", os.path.join(LLVM_BIN, "llvm-objdump"))
    if not os.path.exists(objdump):
        objdump = shutil.which("llvm-objdump")
    assert objdump, "llvm-objdump not found"
    local = os.path.join(str(tmp_path), "gemm_t.o")
    shutil.copy(OBJ, local)
    subprocess.run([objdump, "--offloading", local], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    dev = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(str(tmp_path))
    return objdump, os.path.join(str(tmp_path), dev[0])


def test_kernel_uses_transposed_lds_reads_and_mfma(lib, tmp_path):
    objdump, dev = _device_object(tmp_path)
    text = subprocess.run([objdump, "-d", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert "gemm_t_kernel" in text
    assert re.search(r"\bds_read_b64_tr_b16\b", text)
    assert re.search(r"\bv_mfma_f32_32x32x16_f16\b", text)


def test_kernel_has_no_scratch(lib, tmp_path):
    _, dev = _device_object(tmp_path)
    readelf = os.path.join(LLVM_BIN, "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    notes = subprocess.run([readelf, "--notes", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    kernels = re.split(r"\n\s*- \.", notes)
    meta = [k for k in kernels if "gemm_t_kernel" in k]
    assert meta, "no code-object metadata for gemm_t_kernel"
    for k in meta:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", k), k
        assert re.search(r"\.vgpr_spill_count:\s+0\b", k), k
        assert re.search(r"\.sgpr_spill_count:\s+0\b", k), k


@pytest.mark.parametrize("binding", ["ops", "ops_ctypes"])
def test_operator_rejects_cpu_tensors(lib, binding):
    import importlib

    import torch
    mod = importlib.import_module("eetq_amd." + binding)
    assert "w8_a16_gemm_t" in mod.__all__
    g = torch.zeros(2, 64, dtype=torch.float16)
    w = torch.zeros(128, 64, dtype=torch.int8)
    s = torch.ones(64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        mod.w8_a16_gemm_t(g, w, s)
