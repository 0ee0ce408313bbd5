"""The dense tiled kernel on int4 weights (eetq_w4a16_gemm_tiled) without a GPU: the entry and its shape query are
declared, exported and bound; the query answers from the shapes alone; bad arguments are refused before any launch and name the
entry; both operator modules list the two ops and agree with the C query; W4A16Linear.prompt_path is a plain class attribute (state
dicts unchanged) with one pure routing method, and utils.set_prompt_path sets it; and the launcher's column offset, the weight DMA
and the fragment read, restated in NumPy on the oracle's int4 layout."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eetq_w4a16_gemm_tiled", "eetq_w4a16_gemm_tiled_supported")
ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_entries_declared_exported_and_bound(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert len(lib.eetq_w4a16_gemm_tiled.argtypes) == 11        # eetq_w4a16_gemm_ex's, tile_j in the place of path
    assert len(lib.eetq_w4a16_gemm_tiled_supported.argtypes) == 3
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr and lib.eetq_abi_version() == 7
    mk = open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()
    assert re.search(r"SRCS\s*:=.*\bgemm_int4_tiled\.hip", mk) and re.search(r"HAZARD_CHECKED\s*:=.*\bgemm_int4_tiled\.o", mk)
    assert '"gemm_int4_tiled.o"' in open(os.path.join(ROOT, "tools", "check_store_hazard.floors.json")).read()


def test_support_query_answers_without_a_device(lib):
    f = lib.eetq_w4a16_gemm_tiled_supported
    assert f(200, 384, 384) == 1
    assert f(200, 384, 256) == 0          # K < 384: fewer than six K steps
    assert f(200, 384, 320) == 0          # K % 128 != 0
    assert f(200, 24, 384) == 0           # N % 16 != 0
    assert f(0, 384, 384) == 0
    assert f(200, 65536, 65536) == 0      # N K / 2 = 2^31
    assert f(200, 32768, 65536) == 1
    assert f(1 << 22, 384, 1024) == 1     # 8 GiB of activations: rows go in chunks
    assert f(-1, 384, 384) == 0 and f(200, 0, 384) == 0 and f(200, 384, 0) == 0
    for K in range(64, 1281, 64):
        assert f(300, 512, K) == (1 if K % 128 == 0 and K >= 384 else 0), K


def test_entry_rejects_bad_arguments_without_a_device(lib):
    p, n = ctypes.c_void_p(16), None   # never dereferenced: every case fails its argument check first
    f = lib.eetq_w4a16_gemm_tiled
    ok = [p, p, p, n, n, p, 200, 384, 384, 0, n]   # x, w, scales, bias, residual, y, M, N, K, tile_j, stream
    for i in (0, 1, 2, 5):
        args = list(ok)
        args[i] = n
        assert f(*args) == ERR_INVALID, i
        assert b"eetq_w4a16_gemm_tiled" in lib.eetq_last_error() and b"null" in lib.eetq_last_error()

    def with_(**kw):
        names = ("M", "N", "K", "tile_j")
        a = list(ok)
        for key, v in kw.items():
            a[6 + names.index(key)] = v
        return a
    for tj in (-1, 3):
        assert f(*with_(tile_j=tj)) == ERR_INVALID
        assert b"eetq_w4a16_gemm_tiled: tile_j" in lib.eetq_last_error()
    assert f(*with_(K=448)) == ERR_INVALID
    assert b"eetq_w4a16_gemm_tiled" in lib.eetq_last_error() and b"multiple of 128" in lib.eetq_last_error()
    assert f(*with_(N=200)) == ERR_INVALID
    assert b"eetq_w4a16_gemm_tiled" in lib.eetq_last_error() and b"multiple of 16" in lib.eetq_last_error()
    assert f(*with_(M=0)) == ERR_INVALID
    assert b"eetq_w4a16_gemm_tiled" in lib.eetq_last_error() and b"shape" in lib.eetq_last_error()
    a = list(ok)
    a[0] = ctypes.c_void_p(24)          # misaligned x
    assert f(*a) == ERR_INVALID
    assert b"eetq_w4a16_gemm_tiled" in lib.eetq_last_error() and b"16-byte" in lib.eetq_last_error()
    for i, addr in ((3, 20), (4, 24)):  # bias 8-byte, residual 16-byte
        a = list(ok)
        a[i] = ctypes.c_void_p(addr)
        assert f(*a) == ERR_INVALID and b"eetq_w4a16_gemm_tiled" in lib.eetq_last_error()


def test_both_operator_modules_list_the_ops_and_agree_with_the_query(lib):
    from eetq_amd import ops, ops_ctypes
    for name in ("w4_a16_gemm_tiled", "w4_a16_gemm_tiled_supported"):
        assert name in ops.__all__ and name in ops_ctypes.__all__
        assert callable(getattr(ops, name)) and callable(getattr(ops_ctypes, name))
    f = lib.eetq_w4a16_gemm_tiled_supported
    for M in (1, 128, 129, 4096):
        for N in (16, 24, 384, 11008):
            for K in (128, 256, 320, 384, 448, 512, 4096):
                want = f(M, N, K) == 1
                assert ops.w4_a16_gemm_tiled_supported(M, N, K) == want, (M, N, K)
                assert ops_ctypes.w4_a16_gemm_tiled_supported(M, N, K) == want, (M, N, K)
    assert not ops.w4_a16_gemm_tiled_supported(0, 384, 384) and not ops_ctypes.w4_a16_gemm_tiled_supported(0, 384, 384)
    assert ops.w4_a16_gemm_tiled_supported(200, 384, 384) is True


def test_prompt_path_is_a_class_attribute_with_one_pure_routing_method():
    from eetq_amd.modules.qlinear import W4A16Linear
    assert W4A16Linear.prompt_path == "auto" and W4A16Linear.PROMPT_PATHS == ("auto", "direct")
    lin = torch.nn.Linear(1024, 384, bias=True, dtype=torch.float16)
    mod = W4A16Linear.from_torch(lin, init_only=True)
    assert "prompt_path" not in vars(mod)
    keys = {"qweight", "weight_scales", "bias"}
    assert set(mod.state_dict()) == keys
    assert [mod.route(r) for r in (1, 16, 128, 129, 200, 1 << 20)] == ["auto"] * 6
    mod.prompt_path = "direct"
    assert set(mod.state_dict()) == keys and not list(mod.parameters())
    assert [mod.route(r) for r in (0, 1, 16, 17, 128)] == ["auto"] * 5
    assert [mod.route(r) for r in (129, 200, 4096, 1 << 22)] == ["direct"] * 4
    assert W4A16Linear.prompt_path == "auto"                      # the instance's, not the class's
    shallow = W4A16Linear.from_torch(torch.nn.Linear(256, 64, bias=False, dtype=torch.float16), init_only=True)
    shallow.prompt_path = "direct"
    assert shallow.route(200) == "auto" and shallow.route(4096) == "auto"     # K = 256 < 384: outside the kernel, quietly
    mod.prompt_path = "expand"
    with pytest.raises(ValueError, match="prompt_path"):
        mod.route(200)
    with pytest.raises(ValueError, match="prompt_path"):
        mod.route(1)


def test_set_prompt_path_counts_int4_linears_and_refuses_unknown_paths_first():
    import eetq_amd.utils as utils
    from eetq_amd.modules.qlinear import W4A16Linear, W8A16Linear
    from eetq_amd.utils.quantizer import set_prompt_path
    assert utils.set_prompt_path is set_prompt_path
    f16 = torch.float16
    model = torch.nn.Sequential(W4A16Linear.from_torch(torch.nn.Linear(512, 128, dtype=f16), init_only=True),
                                W8A16Linear.from_torch(torch.nn.Linear(128, 128, dtype=f16), init_only=True),
                                torch.nn.Sequential(W4A16Linear.from_torch(torch.nn.Linear(128, 64, dtype=f16), init_only=True)),
                                torch.nn.Linear(64, 8, dtype=f16))
    int4 = [m for m in model.modules() if isinstance(m, W4A16Linear)]
    assert len(int4) == 2
    assert set_prompt_path(model, "direct") == 2 and all(m.prompt_path == "direct" for m in int4)
    assert not hasattr(model[1], "prompt_path")
    for bad in ("expand", "", None, "DIRECT"):
        with pytest.raises(ValueError, match="set_prompt_path"):
            set_prompt_path(model, bad)
        assert all(m.prompt_path == "direct" for m in int4)
    assert set_prompt_path(model, "auto") == 2 and all(m.prompt_path == "auto" for m in int4)
    assert set_prompt_path(int4[0], "direct") == 1 and int4[1].prompt_path == "auto"   # the model itself included
    import inspect
    assert list(inspect.signature(utils.eet_quantize).parameters)[-1] == "router"


@pytest.mark.parametrize("c0", [0, 64, 128])
def test_column_offset_weight_dma_and_fragment_read_on_the_oracle_layout(c0):
    """launch_gemm_tile_i4 and gemm_tile_body<BITS = 4, GROUPED = false> on the oracle's layout alone.  A launch over the columns
    from c0 starts at weight byte (c0 / 16) (K / 128) 1024 (an int4 tile is 16 columns x 128 k; the int8 layout has K / 64 there).
    Half-wave `lane >> 5` of a weight DMA piece brings, for launch-local column tile nt and K step kt, the 16 bytes at
    nt (KT >> 1) 1024 + kt 512 + (lane & 31) 16 per lane; wave (grp, wn), lane (fn, fh) then reads the 8 bytes at grp 256 +
    (fn & 15) 16 + fh 8 of that half tile: k = 64 kt + 32 grp + 16 fh + [0, 16) of column c0 + 16 nt + (fn & 15), at nibble positions
    [0, 4, 1, 5, 2, 6, 3, 7], stored as q + 8."""
    import oracle
    K, N = 384, 160
    rng = np.random.default_rng(11)
    vals = rng.integers(-8, 8, size=(K, N)).astype(np.int8)
    packed = oracle.gfx950_pack_i4(oracle.i4_from_values(vals)).view(np.uint8).reshape(-1)
    assert packed.size == K * N // 2
    KT = K // 64
    base = (c0 // 16) * (K // 128) * 1024
    launch = packed[base:]
    cols = N - c0
    assert launch.size == cols * K // 2                         # what w_rsrc spans: N K / 2 bytes of this launch's columns
    if c0:
        assert base != (c0 // 16) * (K // 64) * 1024            # the int8 formula is another byte
    pos = [0, 4, 1, 5, 2, 6, 3, 7]
    seen = np.zeros((K, cols), bool)
    for kt in range(KT):
        for nt in range(cols // 16):
            stage = np.empty(512, np.uint8)                     # the half tile one half-wave lands in LDS
            for lane in range(32):
                src = nt * (KT >> 1) * 1024 + kt * 512 + lane * 16
                assert src + 16 <= launch.size
                stage[lane * 16:lane * 16 + 16] = launch[src:src + 16]
            for grp in range(2):
                for fn in range(16):
                    for fh in range(2):
                        at = grp * 256 + fn * 16 + fh * 8
                        dwords = stage[at:at + 8].view("<u4")
                        got = [((int(dwords[j >> 3]) >> (4 * pos[j & 7])) & 0xF) - 8 for j in range(16)]
                        k0 = 64 * kt + 32 * grp + 16 * fh
                        assert k0 == 64 * kt + 32 * grp + 16 * fh and k0 % 64 == 32 * grp + 16 * fh
                        assert got == vals[k0:k0 + 16, c0 + 16 * nt + fn].tolist(), (kt, nt, grp, fn, fh)
                        seen[k0:k0 + 16, 16 * nt + fn] = True
    assert seen.all()   # every weight of the launch's columns is read exactly where some lane expects it
