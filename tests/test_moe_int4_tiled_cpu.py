"""The grouped tiled kernel on int4 expert stacks (path "direct") without a GPU: eetq_w4a16_moe_gemm_tiled and its
shape query are declared, exported and bound; the query answers from the shapes alone; bad arguments are refused before any launch
and name the entry; the compiled module's int4 ops know path="direct" and ops.w4_a16_moe_direct_supported agrees with the C query;
W4A16Experts.prompt_path is a plain attribute (state dicts unchanged) that eet_quantize sets; and the kernel's address arithmetic
for the weight DMA and the fragment read, restated in NumPy on the oracle's int4 layout."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eetq_w4a16_moe_gemm_tiled", "eetq_w4a16_moe_gemm_tiled_supported")
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
    assert len(lib.eetq_w4a16_moe_gemm_tiled.argtypes) == 16     # eetq_w8a16_moe_gemm_tiled's 15 and tile_j
    assert len(lib.eetq_w4a16_moe_gemm_tiled_supported.argtypes) == 6
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr and lib.eetq_abi_version() == 7
    mk = open(os.path.join(ROOT, "eetq_amd", "csrc", "Makefile")).read()
    assert "moe_int4_tiled.hip" in mk and re.search(r"HAZARD_CHECKED\s*:=.*moe_int4_tiled\.o", mk)
    assert "moe_int4_tiled.o" in open(os.path.join(ROOT, "tools", "check_store_hazard.floors.json")).read()


def test_support_query_answers_without_a_device(lib):
    f, f8 = lib.eetq_w4a16_moe_gemm_tiled_supported, lib.eetq_w8a16_moe_gemm_tiled_supported
    assert f(512, 2, 8, 768, 320, 1) == 0 and f8(512, 2, 8, 768, 320, 1) == 1   # K % 128 != 0
    assert f(512, 2, 8, 768, 256, 1) == 0                                        # K < 384
    assert f(512, 2, 8, 768, 384, 1) == 1 and f(512, 2, 8, 768, 384, 0) == 1
    assert f(512, 2, 8, 24, 384, 1) == 0                                         # N % 16 != 0
    assert f(512, 2, 8, 65536, 32768, 1) == 0                                    # N K = 2^31 per expert
    assert f(512, 2, 8, 32768, 32768, 1) == 1
    assert f(1 << 20, 2, 8, 768, 1024, 1) == 0                                   # 2 GiB of activations
    assert f(0, 2, 8, 768, 512, 1) == 0 and f(4, 0, 8, 768, 512, 1) == 0
    for K in range(64, 1281, 64):   # otherwise the int8 rule
        assert f(300, 2, 8, 512, K, 1) == (1 if K % 128 == 0 and K >= 384 and f8(300, 2, 8, 512, K, 1) else 0), K


def test_entry_rejects_bad_arguments_without_a_device(lib):
    p, n = ctypes.c_void_p(16), None   # never dereferenced: every case fails its argument check first
    f = lib.eetq_w4a16_moe_gemm_tiled
    ok = [p, p, p, p, p, p, p, 64, 2, 8, 256, 512, 1, 1, 0, n]
    for i in (0, 1, 2, 3, 5, 6):  # x, w_packed_i4, scales, offsets, active, y
        args = list(ok)
        args[i] = n
        assert f(*args) == ERR_INVALID, i
        assert b"eetq_w4a16_moe_gemm_tiled" in lib.eetq_last_error() and b"null" in lib.eetq_last_error()
    args = list(ok)
    args[4] = n                       # sorted_slot matters when gathering
    assert f(*args) == ERR_INVALID

    def with_(**kw):
        names = ("T", "k", "E", "N", "K", "gather", "glu8", "tile_j")
        a = list(ok)
        for key, v in kw.items():
            a[7 + names.index(key)] = v
        return a
    for tj in (3, -1, 8):
        assert f(*with_(tile_j=tj)) == ERR_INVALID
        assert b"eetq_w4a16_moe_gemm_tiled: tile_j" in lib.eetq_last_error()
    assert f(*with_(k=9)) == ERR_INVALID
    assert b"eetq_w4a16_moe_gemm_tiled: k must be in [1, E]" in lib.eetq_last_error()
    assert f(*with_(T=-1)) == ERR_INVALID
    assert b"eetq_w4a16_moe_gemm_tiled: T must be" in lib.eetq_last_error()
    assert f(*with_(K=448)) == ERR_INVALID and b"K % 128" in lib.eetq_last_error()
    assert f(*with_(N=200)) == ERR_INVALID
    assert f(*with_(gather=2)) == ERR_INVALID and f(*with_(glu8=3)) == ERR_INVALID
    a = list(ok)
    a[0] = ctypes.c_void_p(24)
    assert f(*a) == ERR_INVALID and b"16-byte" in lib.eetq_last_error()


def test_ops_know_the_direct_path():
    from eetq_amd import _lib, ops, ops_ctypes
    assert "w4_a16_moe_direct_supported" in ops.__all__ and "w4_a16_moe_direct_supported" in ops_ctypes.__all__
    if ops.BOUNDARY == "ext":
        for name in ("w4_a16_moe", "w4_a16_moe_block", "w4_a16_moe_block_sigmoid"):
            doc = getattr(ops, name).__doc__
            assert re.search(r"path: str = 'auto'", doc) and "'direct'" in doc, name
        assert ops.w4_a16_moe_path(512, 2, 8, 512, 384) == "expand" and ops.w4_a16_moe_path(64, 2, 8, 512, 384) == "decode"
    f = _lib.lib().eetq_w4a16_moe_gemm_tiled_supported
    for T in (1, 17, 512):
        for k, E in ((2, 8), (8, 128)):
            for H in (128, 256, 320, 384, 512, 1152):
                for I in (128, 384, 448, 768):
                    want = f(T, k, E, 2 * I, H, 1) == 1 and f(T, k, E, H, I, 0) == 1
                    assert ops.w4_a16_moe_direct_supported(T, k, E, H, I) == want, (T, k, E, H, I)
                    assert ops_ctypes.w4_a16_moe_direct_supported(T, k, E, H, I) == want, (T, k, E, H, I)
    assert ops.w4_a16_moe_direct_supported(64, 2, 8, 512, 384) and not ops.w4_a16_moe_direct_supported(64, 2, 8, 128, 128)
    assert not ops.w4_a16_moe_direct_supported(0, 2, 8, 512, 384)


def _mixtral(H=512, I=384):
    from transformers import MixtralConfig, MixtralForCausalLM
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=8, num_experts_per_tok=2, vocab_size=64)
    return MixtralForCausalLM(cfg).half()


def test_prompt_path_is_a_plain_attribute_that_eet_quantize_sets():
    from eetq_amd.modules.qlinear import W4A16Experts
    from eetq_amd.utils.quantizer import eet_quantize
    default, direct = _mixtral(), _mixtral()
    eet_quantize(default, init_only=True, experts=True, expert_bits=4)
    eet_quantize(direct, init_only=True, experts=True, expert_bits=4, expert_prompt_path="direct")
    a, b = default.model.layers[0].mlp.experts, direct.model.layers[0].mlp.experts
    assert type(a) is W4A16Experts and type(b) is W4A16Experts
    assert W4A16Experts.prompt_path == "auto" and a.prompt_path == "auto" and b.prompt_path == "direct"
    keys = {"gate_up_qweight", "gate_up_scales", "down_qweight", "down_scales"}
    assert set(a.state_dict()) == keys and set(b.state_dict()) == keys and not list(b.parameters())
    a.load_state_dict(b.state_dict())
    b.load_state_dict(a.state_dict())
    assert a.prompt_path == "auto" and b.prompt_path == "direct"
    # what the module hands to the op: shapes only.  E 8, k 2, H 512, I 384
    assert a.op_path(1, 2) == a.op_path(64, 2) == a.op_path(4096, 2) == "auto"
    assert b.op_path(16, 2) == "decode"            # T <= 16
    assert b.op_path(17, 2) == "decode"            # 34 slots < 16 E
    assert b.op_path(63, 2) == "decode" and b.op_path(64, 2) == "direct" and b.op_path(4096, 2) == "direct"
    small = _mixtral(H=128, I=256)
    eet_quantize(small, init_only=True, experts=True, expert_bits=4, expert_prompt_path="direct")
    assert small.model.layers[0].mlp.experts.op_path(4096, 2) == "decode"   # K = 128 < 384: never the expansion in this mode
    b.prompt_path = "expand"
    with pytest.raises(ValueError, match="prompt_path"):
        b.op_path(64, 2)


@pytest.mark.parametrize("kwargs", [{"expert_prompt_path": "expand"}, {"expert_prompt_path": "direct", "expert_bits": 8},
                                    {"expert_prompt_path": None}])
def test_bad_expert_prompt_path_raises_before_the_model_is_touched(kwargs):
    from eetq_amd.utils.quantizer import eet_quantize
    model = _mixtral(H=128, I=128)
    before = [(n, type(m), id(m)) for n, m in model.named_modules()]
    with pytest.raises(ValueError, match="expert_prompt_path"):
        eet_quantize(model, init_only=True, **dict({"experts": True, "expert_bits": 4}, **kwargs))
    assert [(n, type(m), id(m)) for n, m in model.named_modules()] == before


def test_lane_mapping_of_the_int4_tile_body_on_the_oracle_layout():
    """gemm_tile_body<BITS = 4> on the oracle's layout alone.  K step kt of column tile nt is the 512 bytes at kt * 512 of the
    tile's row of 1 KiB tiles (K * 8 bytes per column tile).  Wave (grp, wn), lane (fn, fh) of a J-block tile reads 8 bytes at
    tile * 512 + grp * 256 + (fn & 15) * 16 + fh * 8 of the stage: they must hold k = 64 kt + 32 grp + 16 fh + [0, 16) of its
    column, dword d the eight k of MFMA e = d, at nibble positions [0, 4, 1, 5, 2, 6, 3, 7], stored as q + 8."""
    import oracle
    K, N = 384, 48
    rng = np.random.default_rng(7)
    vals = rng.integers(-8, 8, size=(K, N)).astype(np.int8)
    packed = oracle.gfx950_pack_i4(oracle.i4_from_values(vals)).view(np.uint8).reshape(-1)
    assert packed.size == K * N // 2
    assert np.array_equal(oracle.i4_values(oracle.gfx950_unpack_i4(packed.view(np.int8).reshape(K, N // 2))), vals)
    pos = [0, 4, 1, 5, 2, 6, 3, 7]
    row_bytes = (K // 128) * 1024
    seen = np.zeros((K, N), bool)
    for kt in range(K // 64):
        for nt in range(N // 16):
            half = packed[nt * row_bytes + kt * 512: nt * row_bytes + (kt + 1) * 512]   # what one half-wave DMA brings
            for grp in range(2):
                for fn in range(16):
                    for fh in range(2):
                        at = grp * 256 + fn * 16 + fh * 8
                        dwords = half[at:at + 8].view("<u4")
                        got = [((int(dwords[j >> 3]) >> (4 * pos[j & 7])) & 0xF) - 8 for j in range(16)]
                        k0 = 64 * kt + 32 * grp + 16 * fh
                        col = 16 * nt + fn
                        assert got == vals[k0:k0 + 16, col].tolist(), (kt, nt, grp, fn, fh)
                        seen[k0:k0 + 16, col] = True
    assert seen.all()   # every weight is read exactly where some lane expects it
    # the dequant's extraction: ((w >> 4 i) & 0x000f000f) | 0x64006400 is the fp16 pair (k 2 i, 2 i + 1) + 1024
    w = int(packed[:4].view("<u4")[0])
    for i in range(4):
        pair = np.array([((w >> (4 * i)) & 0x000F000F) | 0x64006400], np.uint32).view(np.float16)
        assert (pair - np.float16(1032)).tolist() == vals[2 * i:2 * i + 2, 0].astype(np.float16).tolist()
