"""The launch plan of the LDS-tiled MFMA GEMM (eetq_amd/csrc/gemm_tile_plan.hpp) through eetq_diag_tile_plan: host arithmetic only,
`cus` always given, so no device is asked.  The planner is held against act_cases.mfma_launches / ragged_round_slices, the
independent restatement of the rule the launchers had before they shared one planner."""
import ctypes
import itertools
import os
import shutil
import subprocess

import pytest

import act_cases
from conftest import ROOT

CUS = (256, 304, 64, 8, 1)
MS = (1, 127, 128, 129, 256, 512, 1000, 1024, 4096, 20000)
NS = (16, 64, 80, 128, 2176, 4096, 5120, 11008, 13824, 32896)
KS8 = (272, 320, 384, 4096, 5056, 5120, 13824)
KS4 = tuple(K for K in KS8 if K % 128 == 0 and K >= 384)
TILE = {2: "wide", 1: "narrow", 0: "stream"}
UNSUPPORTED, INVALID = -3, -1


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def plan(lib, bits, M, N, K, act=0, tile_j=0, cus=256, max_records=320):
    """(status, records [(row0, rows, col0, cols, tile, k_slices)] that were filled, *count)"""
    rec = (ctypes.c_int * (6 * max_records))(*([-9] * (6 * max_records)))
    count = ctypes.c_int(-9)
    rc = lib.eetq_diag_tile_plan(bits, M, N, K, act, tile_j, cus, rec, max_records, ctypes.byref(count))
    filled = [tuple(rec[6 * i:6 * i + 6]) for i in range(max_records) if rec[6 * i] != -9]
    return rc, filled, count.value


def as_launches(records):
    """act_cases.mfma_launches' form: (tile, first column or row, columns or rows)"""
    return [(TILE[t], r0, rows) if t == 0 else (TILE[t], c0, cols) for r0, rows, c0, cols, t, _ in records]


def test_launches_and_slices_over_the_grid(lib):
    """Every launch list equals the restated rule; the ragged round asks for two K slices exactly where the restatement does under
    the int8 identity epilogue, and for one everywhere else; int4 never reaches the stream kernel."""
    seen = {"stream": 0, "two": 0, "sliced": 0}
    for bits, ks in ((8, KS8), (4, KS4)):
        for cus, M, N, K, act in itertools.product(CUS, MS, NS, ks, (0, 1)):
            if bits == 4 and act:
                continue   # refused: test_refusals
            rc, recs, count = plan(lib, bits, M, N, K, act=act, cus=cus)
            where = (bits, cus, M, N, K, act)
            assert rc == 0 and count == len(recs), where
            assert as_launches(recs) == act_cases.mfma_launches(M, N, K, cus), where
            assert all((r[0], r[1]) == (0, M) for r in recs if r[4] != 0), where          # one row chunk: all rows in every launch
            assert all((r[2], r[3]) == (0, N) for r in recs if r[4] == 0), where          # a stream chunk takes all columns
            want = [1] * len(recs)
            if len(recs) == 2 and recs[0][4] != 0 and act == 0 and bits == 8:
                want[1] = act_cases.ragged_round_slices(M, N, K, cus)
            assert [r[5] for r in recs] == want, where
            assert bits == 8 or all(r[4] != 0 for r in recs), where
            seen["stream"] += recs[0][4] == 0
            seen["two"] += len(recs) == 2 and recs[0][4] != 0
            seen["sliced"] += recs[-1][5] == 2
    assert min(seen.values()) > 0, seen   # the grid reaches every kind of plan


def test_ragged_round_in_two_k_slices(lib):
    """M = 1024 at 5120 x 5120 on 256 CUs: 256 wide tiles, then 128 narrow tiles in 2 K slices under the identity epilogue."""
    assert plan(lib, 8, 1024, 5120, 5120)[1] == [(0, 1024, 0, 4096, 2, 1), (0, 1024, 4096, 1024, 1, 2)]
    assert plan(lib, 8, 1024, 5120, 5120, act=1)[1] == [(0, 1024, 0, 4096, 2, 1), (0, 1024, 4096, 1024, 1, 1)]
    assert plan(lib, 4, 1024, 5120, 5120)[1] == [(0, 1024, 0, 4096, 2, 1), (0, 1024, 4096, 1024, 1, 1)]


@pytest.mark.parametrize("bits", [8, 4])
def test_pinned_plans_at_256_cus(lib, bits):
    assert plan(lib, bits, 200, 384, 1024)[1] == [(0, 200, 0, 384, 1, 1)]
    assert plan(lib, bits, 1024, 2176, 384)[1] == [(0, 1024, 0, 2176, 2, 1)]      # 136 wide tiles against 272 narrow
    assert plan(lib, bits, 1024, 5120, 384)[1] == [(0, 1024, 0, 4096, 2, 1), (0, 1024, 4096, 1024, 1, 1)]


@pytest.mark.parametrize("bits", [8, 4])
def test_row_chunks(lib, bits):
    """The only place the loop over row chunks is exercised: no GPU test covers it, because the smallest case needs more than 2 GiB
    of activations.  K = 65536: 16256 rows per launch, so M = 16257 leaves one row for a second chunk."""
    assert plan(lib, bits, 16257, 16, 65536)[1] == [(0, 16256, 0, 16, 1, 1), (16256, 1, 0, 16, 1, 1)]
    # K = 384: 2796160 rows per launch.  M = 2^22 is two launches (a chunk of more row tiles than CUs is never cut along its columns),
    # so *count exceeds max_records only below 2; M = 2^24 is seven, which exceeds a max_records of 4
    rows = ((2 ** 31 - 1) // (2 * 384)) // 128 * 128
    rc, recs, count = plan(lib, bits, 1 << 22, 16, 384, max_records=1)
    assert rc == 0 and count == 2 and [(r[0], r[1]) for r in recs] == [(0, rows)]
    rc, recs, count = plan(lib, bits, 1 << 24, 16, 384, max_records=4)
    assert rc == 0 and count == -(-(1 << 24) // rows) == 7 and [(r[0], r[1]) for r in recs] == [(i * rows, rows) for i in range(4)]
    assert plan(lib, bits, 1 << 24, 16, 384)[1][-1][:2] == (6 * rows, (1 << 24) - 6 * rows)


def test_forced_shape(lib):
    assert plan(lib, 4, 1024, 5120, 384, tile_j=1)[1] == [(0, 1024, 0, 5120, 1, 1)]
    assert plan(lib, 4, 1024, 5120, 384, tile_j=2)[1] == [(0, 1024, 0, 5120, 2, 1)]
    assert plan(lib, 4, 1024, 5120, 384, tile_j=2, cus=0)[1] == [(0, 1024, 0, 5120, 2, 1)]   # forced: no device is asked
    assert plan(lib, 4, 16257, 16, 65536, tile_j=2)[1] == [(0, 16256, 0, 16, 2, 1), (16256, 1, 0, 16, 2, 1)]


def test_refusals(lib):
    count, rec = ctypes.c_int(0), (ctypes.c_int * 12)()
    assert lib.eetq_diag_tile_plan(8, 256, 256, 384, 0, 0, 256, None, 2, ctypes.byref(count)) == INVALID
    assert lib.eetq_diag_tile_plan(8, 256, 256, 384, 0, 0, 256, rec, 2, None) == INVALID
    assert plan(lib, 5, 256, 256, 384)[0] == INVALID
    assert b"eetq_diag_tile_plan" in lib.eetq_last_error()
    for bits, M, N, K, act, tile_j in ((4, 256, 256, 320, 0, 0), (4, 256, 256, 272, 0, 0), (4, 256, 256, 384, 1, 0),
                                       (4, 256, 256, 384, 0, 3), (8, 256, 256, 384, 0, 3), (8, 256, 256, 65536 * 128, 0, 0)):
        assert plan(lib, bits, M, N, K, act=act, tile_j=tile_j)[0] == UNSUPPORTED, (bits, M, N, K, act, tile_j)
        assert b"eetq_diag_tile_plan" in lib.eetq_last_error()


PROBE = """
#include "gemm_tile_plan.hpp"
using namespace eetq::tile_plan;
extern "C" long probe_grouped_row_tiles(int S, int E) { return grouped_row_tiles(S, E); }
extern "C" int probe_grouped_narrow(int S, int E, int N, int cus) { return narrow_cheaper(grouped_row_tiles(S, E), N, cus); }
"""


def test_grouped_rule_is_the_dense_rule(lib, tmp_path):
    """What moe_tiled_narrow computes (gemm_tile_plan.hpp compiled on its own by the host compiler: it needs no HIP) is the dense cost
    rule at tiles_m = min(E, S) * ceil(ceil(S / min(E, S)) / 128) -- restated here, and read back from the dense plan wherever that
    plan is one unforced launch."""
    cxx = shutil.which("g++") or shutil.which("c++")
    src, so = tmp_path / "probe.cpp", tmp_path / "probe.so"
    src.write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "eetq_amd", "csrc"), str(src), "-o", str(so)],
                   check=True)
    probe = ctypes.CDLL(str(so))
    probe.probe_grouped_row_tiles.restype = ctypes.c_long
    read_back = 0
    for S, E, N, cus in itertools.product((1, 3, 127, 128, 129, 660, 1024, 4096, 20000), (1, 4, 8, 64, 256), (16, 64, 384, 768, 2176, 4096, 5120),
                                          (256, 64, 8)):
        A = min(E, S)
        tiles_m = A * -(-(-(-S // A)) // 128)
        assert probe.probe_grouped_row_tiles(S, E) == tiles_m, (S, E)
        t2, t1 = tiles_m * -(-N // 128), tiles_m * -(-N // 64)
        want = 0.70 * -(-t1 // cus) < -(-t2 // cus)
        assert bool(probe.probe_grouped_narrow(S, E, N, cus)) == want, (S, E, N, cus)
        recs = plan(lib, 4, 128 * tiles_m, N, 384, cus=cus)[1]
        if len(recs) == 1:
            assert (recs[0][4] == 1) == want, (S, E, N, cus)
            read_back += 1
    assert read_back > 100
