"""Inputs, reference, mutants and the table of cases of tests/test_gpu_exact_sums.py: "fp32 accumulation, one rounding" of the
W8A16 / W4A16 contract y = fp16(sum_k fp32(x) fp32(fp16(q s))), held bit for bit in every dense kernel form.  NumPy only, no GPU.

Exact-sum inputs.  x[m, k] = i / 4 with i an integer in -A .. A; s[n] = c 2^-e with c in {1, 1.25, 1.5, 1.75} (c4 = 4 c in 4 .. 7) and e
in 6 .. 9; q every int8 code (every nibble for int4).  q c4 <= 896 < 2^11, so fp16(q s) = q c4 2^-(e + 2) exactly, and every product
x fp16(q s) = i q c4 2^-(e + 4) is an integer number of quanta 2^-(e + 4).  No activation and no dequantised weight is an fp16
subnormal (|q s| >= 2^-9, |x| >= 2^-2 or 0).  THE CONDITION: sum_k |i q c4| < 2^24 for every (m, n), from the actual data.  Then every
partial sum of every subset of the products is an integer below 2^24 quanta, i.e. exactly representable in fp32: every kernel,
whatever its order, K slices, rings, reduction trees or MFMA internals, holds the same accumulator, and its result must equal
fp16(exact sum) as a number on every element.  The input gradient dx = dy fp16(q s)^T sums over n, where the scales vary: its quantum
is that of the smallest scale, 2^-13, and a product is i q c4 2^(9 - e) quanta.

A is 4 for int8 codes and 64 for nibbles (so that |i q| reaches 512 either way and K / 4-deep partial sums do not fit fp16's 11 bits
-- else the fp16-partial mutants below would be invisible on int4 weights); LADDER lowers A and narrows the scales where K (or N
for the gradient) would break the condition.  The level is chosen from the shape alone (expected sum with a 12 % margin) and the
condition is then asserted from the data: tests/test_exact_cases_cpu.py.

The reference is float64 arithmetic on the integers (exact: everything stays far below 2^53), rounded once, float64 -> fp16.
tests/test_exact_cases_cpu.py proves what the GPU assertions rest on: the condition, the exactness of fp16(q s), the oracle and an fp32
product in three k orders agreeing with the reference bit for bit, every mutant visible on >= 5 % of a case's elements while tier A
accepts the early roundings and a lost or doubled product somewhere, and that each shape selects the kernel form it is listed for on
an MI355X (256 CUs).  x = 0 is among the
activations (at K = 65536 the condition cannot be met without it), so a mutant that loses or doubles one product takes a k at which
the rows are non-zero (Problem.loud)."""
import ctypes
from collections import namedtuple

import numpy as np

import act_cases as ac

NCU = ac.NCU
GEMV, MFMA, STREAM, MID, SPLITK, TILESPLIT = ac.GEMV, ac.MFMA, ac.STREAM, ac.MID, ac.SPLITK, ac.TILESPLIT
LIMIT = 2 ** 24              # quanta: below it every integer is an fp32 value
MUTANT_FLOOR = ac.MUTANT_FLOOR

# id; family: the GPU test that runs it; bits: 8 / 4; op: "gemm" (ops.w8_a16_gemm on an int8 or int4 weight), "tiled4"
# (ops.w4_a16_gemm_tiled, arg = tile), "grouped" (ops.w8_a16_gemv_grouped, arg = problems, each 1 x K x N), "gemm_t" (the input
# gradient: dy [M, N] -> dx [M, K]); path / plan: as act_cases.Case; form: the kernel form in words; select: what check_selection
# holds the shape to; twin: the case also runs through the ctypes binding
Case = namedtuple("Case", "id family bits op M K N path plan form select twin arg")


def _case(id, family, M, K, N, path, form, select, bits=8, op="gemm", plan=None, twin=False, arg=None):
    return Case(id, family, bits, op, M, K, N, path, plan, form, select, twin, arg)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _from_act(family, cases, twin_id):
    """The shapes of act_cases under the IDENTITY epilogue: select = ("act", the act_cases case), see check_selection."""
    return [_case(c.id, family, c.M, c.K, c.N, c.path, c.form, ("act", c), plan=c.plan, twin=c.id == twin_id) for c in cases]


# Tiled kernel.  Under the identity epilogue tile-ragged-round runs its second launch in TWO K slices, guard-tilesplit-256 the K-sliced
# tiled kernel at 2 slices and guard-auto-128 (AUTO) at 4: the K-half and slice combines.
TILED = _from_act("tiled", ac.TILED + ac.ACT_GUARDS, "tile-narrow-act")
# ... and one form no act_cases shape reaches: TWO K slices of the 128 x 128 tile (gemm.hip::wide_tile_splitk_slices: 64 KiB partial
# tiles handed over).  4 x 17 = 68 wide tiles fill a quarter to a half of 256 CUs, the 136 narrow ones are too many to slice, and
# K / 64 / 2 = 80 steps per slice is the least the rule takes.
TILED.append(_case("tile-wide-2-slices", "tiled", 512, 10240, 2176, "auto", "AUTO: the 128 x 128 tile in two K slices of 80 steps", ("auto_wide", (TILESPLIT, 2))))
SPLITK_CASES = _from_act("splitk", ac.SPLITK_CASES, "splitk-50-2_2_22")
MID_CASES = _from_act("mid", ac.MID_CASES, "mid-33")
STREAM_CASES = _from_act("stream", ac.STREAM_CASES, "stream-ring16-w8-m12")
GEMV_CASES = _from_act("gemv", ac.GEMV_CASES, "gemv-units8")

# Grouped GEMV (gemv.hip::launch_gemv_grouped; grouped_bodies below restates it): one dispatch holds at most 32 problems and runs the
# 8-wave body with MORE than two tile rows per CU (> 512 rows), the 16-wave bodies below.  N = 272 is 17 tile rows per problem: 4
# problems = 68 rows, 32 problems = 544 rows -- the smallest N % 16 == 0 with 32 N / 16 > 512 (N = 256 gives exactly 512: 16 waves).
GROUPED_CASES = [
    _case("grouped-4-w16", "grouped", 1, 2048, 272, None, "one dispatch of 4 problems, 68 tile rows: 16-wave body, XV = 1", ("grouped", [("w16", 1)]),
          op="grouped", arg=4, twin=True),
    _case("grouped-4-w16-line", "grouped", 1, 4096, 272, None, "one dispatch of 4 problems at K = 4096: 16-wave straight-line body",
          ("grouped", [("w16_line", 1)]), op="grouped", arg=4),
    _case("grouped-32-w8", "grouped", 1, 2048, 272, None, "one dispatch of 32 problems, 544 tile rows: 8-wave body, XV = 1", ("grouped", [("w8", 1)]),
          op="grouped", arg=32),
]

# Deep K (tests/test_gpu_deep_k.py): one shape per instantiation reached above K = 16384.  select "gemv_xv": (act_cases.gemv_form, XV =
# 16-byte activation loads per thread, restated by gemv_xv below).
DEEP_CASES = [
    _case("deep-gemv-units8-xv8", "deep_k", 1, 28672, 64, "auto", "8-column units, XV = 8", ("gemv_xv", ("units8", 8)), twin=True),
    _case("deep-gemv-units884-xv8", "deep_k", 1, 28672, 5120, "auto", "8 + 8 + 4 column units, XV = 8", ("gemv_xv", ("units884", 8))),
    _case("deep-gemv-w16-xv4", "deep_k", 1, 28736, 64, "auto", "K / 64 odd: 16-wave generic form, XV = 4", ("gemv_xv", ("generic16", 4))),
    _case("deep-gemv-w8-xv8", "deep_k", 1, 28672, 8208, "auto", "513 tile rows: 8-wave generic form, XV = 8", ("gemv_xv", ("generic8", 8))),
    _case("deep-gemv-w16-xv8-105k", "deep_k", 1, 53248, 64, "auto", "16-wave generic form, XV = 8, 105 KiB of LDS", ("gemv_xv", ("generic16", 8))),
    _case("deep-gemv-w16-xv8-last-k", "deep_k", 1, 65536, 64, "auto", "the last K the GEMV stages: XV = 8, 129 KiB of LDS", ("gemv_xv", ("generic16", 8))),
    _case("deep-gemv-w16-many-rows", "deep_k", 1, 32832, 8208, "auto", "513 tile rows past the 8-wave staging limit: 16 waves, XV = 8",
          ("gemv_xv", ("generic16", 8))),
    _case("deep-gemv-m2-xv8", "deep_k", 2, 28672, 64, "gemv", "M = 2, 16 waves, XV = 8, 114 KiB of LDS", ("gemv_xv", ("generic16", 8))),
    _case("deep-gemv-m3-xv8", "deep_k", 3, 21760, 64, "gemv", "M = 3, 16 waves, XV = 8, 130.5 KiB", ("gemv_xv", ("generic16", 8))),
    _case("deep-gemv-m4-xv8", "deep_k", 4, 16384, 64, "gemv", "M = 4, 16 waves, XV = 8, 132 KiB: the most the GEMV stages", ("gemv_xv", ("generic16", 8))),
    _case("deep-stream-m1-past-gemv", "deep_k", 1, 65600, 64, "auto", "past every GEMV form: the stream kernel with one row", ("stream", (2, 1, 16))),
    _case("deep-stream-ring8", "deep_k", 2, 28672, 64, "auto", "8-row ring, 16 waves, 448 K steps", ("stream", (2, 1, 16))),
    _case("deep-stream-ring16", "deep_k", 16, 28672, 64, "stream", "16-row ring, 8 waves (AUTO: split-K tile)", ("stream_forced", (2, 1, 8))),
    _case("deep-stream-ring32", "deep_k", 17, 28672, 64, "stream", "32-row ring", ("stream_big", (2, 1, 8))),
    _case("deep-stream-regs-m33", "deep_k", 33, 28672, 64, "stream", "three row tiles, deep-K register form", ("stream_big", (0, 1, 16))),
    _case("deep-stream-regs-nt2", "deep_k", 3, 28672, 4128, "auto", "registers, two tile rows, 8 waves", ("stream", (0, 2, 8))),
    _case("deep-stream-ring16-nt2", "deep_k", 16, 28672, 4128, "auto", "16-row ring, two tile rows", ("stream", (2, 2, 8))),
    # N = 272, K / 64 = 448: four K slices are 112 steps each
    _case("deep-splitk-auto-64", "deep_k", 64, 28672, 272, "auto", "AUTO: split-K tile, 4 K slices x 2 row groups, ring 33", ("auto_plan", ((SPLITK, 2), (1, 4, 33, 2)))),
    _case("deep-splitk-64-2_2_22", "deep_k", 64, 28672, 272, "splitk", "split-K tile, 64-column blocks, 2 K slices of 56 steps", ("splitk_plan", (2, 2, 22)), plan="2,2,22"),
    _case("deep-splitk-128-1_4_22", "deep_k", 128, 28672, 272, "splitk", "split-K tile, 4 K slices of 28 steps, MT = 4", ("splitk_plan", (1, 4, 22)), plan="1,4,22"),
    _case("deep-splitk-128-2_4_22_2", "deep_k", 128, 28672, 272, "splitk", "split-K tile, 4 K slices x 2 row groups", ("splitk_plan", (2, 4, 22, 2)), plan="2,4,22,2"),
    _case("deep-mid-64", "deep_k", 64, 28672, 272, "mid", "round-1 tile, 448 K steps", ("none", None)),
    _case("deep-tilesplit-auto-128", "deep_k", 128, 28672, 272, "auto", "AUTO: K-sliced tiled kernel, 4 slices of 112 steps", ("auto", (TILESPLIT, 4))),
    _case("deep-tilesplit-200", "deep_k", 200, 28672, 272, "tilesplit", "K-sliced tiled kernel, 4 slices, two row tiles", ("auto", (TILESPLIT, 4))),
    _case("deep-tile-200", "deep_k", 200, 28672, 272, "mfma", "unsplit narrow tiles, 448 K steps", ("tile_plan", (0, [("narrow", 0, 272, 1)]))),
    _case("deep-grouped-40", "deep_k", 1, 28672, 272, None, "two dispatches: 32 problems on the 8-wave body (XV = 8), then 8 on the 16-wave body (XV = 4)",
          ("grouped", [("w8", 8), ("w16", 4)]), op="grouped", arg=40),
    # int4 tiles (128 k each)
    _case("deep-i4-gemv-units-xv8", "deep_k", 1, 28672, 64, "gemv", "int4 8-column units, XV = 8", ("gemv_i4", ("units8", 8)), bits=4),
    _case("deep-i4-gemv-m2-xv8", "deep_k", 2, 28672, 64, "gemv", "int4 M = 2, 16 waves x 4 tiles, XV = 8", ("gemv_i4", ("generic16x4", 8)), bits=4),
    _case("deep-i4-gemv-last-k", "deep_k", 1, 65536, 64, "gemv", "int4 16 waves x 4 tiles at the last staged K, XV = 8", ("gemv_i4", ("generic16x4", 8)), bits=4),
    _case("deep-i4-stream-m1", "deep_k", 1, 53248, 64, "auto", "int4 AUTO at M = 1: stream kernel, 4-row ring", ("stream", (2, 1, 16)), bits=4),
    _case("deep-i4-stream-m16", "deep_k", 16, 28672, 64, "auto", "int4 16-row ring, 8 waves", ("stream", (2, 1, 8)), bits=4),
    _case("deep-i4-splitk-auto-40", "deep_k", 40, 28672, 64, "auto", "int4 AUTO: split-K tile on the planner's plan", ("auto_i4", SPLITK), bits=4),
    _case("deep-i4-splitk-128-2_4_22_2", "deep_k", 128, 28672, 64, "splitk", "int4 split-K tile, 4 K slices x 2 row groups", ("splitk_plan", (2, 4, 22, 2)),
          bits=4, plan="2,4,22,2"),
    _case("deep-i4-expand-200", "deep_k", 200, 28672, 64, "auto", "int4 AUTO at M = 200: expansion, then the K-sliced tiled kernel", ("expand", (TILESPLIT, 4)), bits=4),
    # the input gradient reduces over N: N = 28672 is 448 steps of 64
    _case("deep-grad-i8-n28672", "deep_k", 17, 320, 28672, None, "w8_a16_gemm_t over N = 28672", ("none", None), op="gemm_t"),
    _case("deep-grad-i4-n28672", "deep_k", 17, 384, 28672, None, "w4_a16_gemm_t over N = 28672", ("none", None), op="gemm_t", bits=4),
]

# W4A16.  GEMV forms: gemv.hip::launch_m_i4, restated by gemv_form_i4; stream forms: eetq_diag_stream_plan with bits = 4
# (streamk.hip::pick_plan_i4: rings need K >= 4096); split-K plans forced as for int8, K = 2176 = 17 int4 tiles (the last step 128 deep)
W4_CASES = [
    _case("i4-gemv-units8", "w4a16", 1, 5120, 272, "auto", "int4 8-column units (K / 128 = 40)", ("gemv_i4", ("units8", 2)), bits=4),
    _case("i4-gemv-k4096-w8", "w4a16", 1, 4096, 8208, "auto", "int4 K = 4096, 513 tile rows: 8-wave generic form", ("gemv_i4", ("k4096_w8", 1)), bits=4),
    _case("i4-gemv-line32", "w4a16", 1, 4096, 272, "auto", "int4 K = 4096 straight-line, activations in registers", ("gemv_i4", ("line32", 0)), bits=4),
    _case("i4-gemv-line64-m2", "w4a16", 2, 8192, 272, "gemv", "int4 M = 2, K = 8192 straight-line", ("gemv_i4", ("line64", 0)), bits=4),
    _case("i4-gemv-generic16x4-m3", "w4a16", 3, 8192, 272, "gemv", "int4 M = 3, 16 waves x 4 tiles", ("gemv_i4", ("generic16x4", 4)), bits=4),
    _case("i4-gemv-generic16x2-m3", "w4a16", 3, 4096, 272, "gemv", "int4 M = 3, 16 waves x 2 tiles", ("gemv_i4", ("generic16x2", 2)), bits=4),
    _case("i4-gemv-shallow8", "w4a16", 1, 2048, 272, "auto", "int4 shallow form, 8 waves", ("gemv_i4", ("shallow8", 1)), bits=4),
    _case("i4-gemv-shallow4-m4", "w4a16", 4, 512, 272, "gemv", "int4 M = 4, shallow form, 4 waves", ("gemv_i4", ("shallow4", 1)), bits=4),
    _case("i4-gemv-shallow1", "w4a16", 1, 128, 272, "auto", "int4 shallow form, 1 wave", ("gemv_i4", ("shallow1", 1)), bits=4),
    _case("i4-stream-ring4", "w4a16", 3, 4096, 272, "auto", "int4 4-row ring, 16 waves", ("stream", (2, 1, 16)), bits=4),
    _case("i4-stream-ring8", "w4a16", 5, 4096, 272, "auto", "int4 8-row ring, 16 waves", ("stream", (2, 1, 16)), bits=4),
    _case("i4-stream-ring16", "w4a16", 9, 4096, 272, "auto", "int4 16-row ring, 8 waves", ("stream", (2, 1, 8)), bits=4),
    _case("i4-stream-ring16-nt2", "w4a16", 12, 4096, 4128, "auto", "int4 16-row ring, two tile rows", ("stream", (2, 2, 8)), bits=4),
    _case("i4-stream-ring-nt2-w16", "w4a16", 3, 8320, 4128, "auto", "int4 4-row ring, two tile rows, 16 waves (K > 8192)", ("stream", (2, 2, 16)), bits=4),
    _case("i4-stream-regs-nt2-w16", "w4a16", 3, 4096, 4128, "auto", "int4 registers, two tile rows, 16 waves", ("stream", (0, 2, 16)), bits=4),
    _case("i4-stream-regs-w8", "w4a16", 3, 4096, 4112, "auto", "int4 registers, one tile row, 8 waves", ("stream", (0, 1, 8)), bits=4),
    _case("i4-stream-regs-nt2-w8", "w4a16", 3, 4096, 8192, "auto", "int4 registers, two tile rows, 8 waves", ("stream", (0, 2, 8)), bits=4),
    _case("i4-stream-block-copy", "w4a16", 3, 4096, 8208, "auto", "int4 block copy", ("stream", (1, 1, 8)), bits=4),
    _case("i4-stream-ring8-w8", "w4a16", 6, 4096, 8208, "auto", "int4 8-row ring, 8 waves", ("stream", (2, 1, 8)), bits=4),
    _case("i4-stream-ring4-w8", "w4a16", 3, 5120, 16400, "auto", "int4 4-row ring, 8 waves (more than four tile rows per CU)", ("stream", (2, 1, 8)), bits=4),
    _case("i4-stream-ring8-nt2", "w4a16", 5, 8192, 16416, "auto", "int4 8-row ring, two tile rows, 8 waves", ("stream", (2, 2, 8)), bits=4),
    _case("i4-stream-shallow-w8", "w4a16", 5, 2048, 272, "auto", "int4 shallow 8-wave register form", ("stream", (0, 1, 8)), bits=4),
    _case("i4-stream-shallow-w4", "w4a16", 5, 512, 272, "auto", "int4 shallow four-wave form", ("stream", (0, 1, 4)), bits=4),
    _case("i4-stream-shallow-w1", "w4a16", 5, 128, 272, "auto", "int4 shallow one-wave form", ("stream", (0, 1, 1)), bits=4),
    _case("i4-splitk-auto-17", "w4a16", 17, 2176, 272, "auto", "int4 AUTO at M = 17: split-K tile on the planner's plan", ("auto_i4", SPLITK), bits=4),
]
for _M, _plans in ((17, [(1, 1, 22), (2, 1, 33)]), (50, [(2, 2, 22), (1, 2, 33)]), (80, [(1, 4, 22)]), (128, [(1, 1, 22), (2, 2, 22, 2), (1, 1, 33, 4)])):
    for _p in _plans:
        W4_CASES.append(_case("i4-splitk-%d-%s" % (_M, "_".join(map(str, _p))), "w4a16", _M, 2176, 272, "splitk",
                              "int4 split-K tile, %d-column blocks, %d K slice(s), ring %d, %d row group(s)" % (32 * _p[0], _p[1], _p[2], _p[3] if len(_p) > 3 else 1),
                              ("splitk_plan", _p), bits=4, plan=",".join(map(str, _p))))
W4_CASES += [
    # w4_a16_gemm_tiled: K = 1152 is nine int4 tiles (an odd count), N = 272 leaves a 16-wide last column tile, M = 129 a one-row last row tile
    _case("i4-tiled-rule", "w4a16", 129, 1152, 272, None, "int4 tiled kernel, tile = 0: the launcher's rule (narrow here)", ("tile_plan", (0, [("narrow", 0, 272, 1)])),
          bits=4, op="tiled4", arg=0, twin=True),
    _case("i4-tiled-narrow", "w4a16", 129, 1152, 272, None, "int4 tiled kernel, tile = 1: 128 x 64", ("tile_plan", (1, [("narrow", 0, 272, 1)])), bits=4, op="tiled4", arg=1),
    _case("i4-tiled-wide", "w4a16", 129, 1152, 272, None, "int4 tiled kernel, tile = 2: 128 x 128", ("tile_plan", (2, [("wide", 0, 272, 1)])), bits=4, op="tiled4", arg=2),
    _case("i4-expand-mfma-200", "w4a16", 200, 1152, 272, "mfma", "the expansion route: nibbles -> int8 tiles, then the W8A16 AUTO launch", ("expand", None), bits=4),
]

# Input gradient: (K, N) = (320, 272) has both tails (K % 128 == 64, N % 64 == 16); the int4 layout needs K % 128 == 0, so
# w4_a16_gemm_t takes (384, 272) as tests/test_gpu_deep_k.py does
GRAD_CASES = []
for _bits, _K in ((8, 320), (4, 384)):
    for _M in (1, 2, 7, 16, 17, 64, 128, 129, 300):
        GRAD_CASES.append(_case("grad-i%d-%dx272-m%d" % (_bits, _K, _M), "gradient", _M, _K, 272, None, "w%d_a16_gemm_t, both tails" % _bits, ("none", None),
                                bits=_bits, op="gemm_t", twin=_M == 17))
    for _M in (1, 17, 129):
        GRAD_CASES.append(_case("grad-i%d-4096x4096-m%d" % (_bits, _M), "gradient", _M, 4096, 4096, None, "w%d_a16_gemm_t, 64 steps over N" % _bits, ("none", None),
                                bits=_bits, op="gemm_t"))

CASES = TILED + SPLITK_CASES + MID_CASES + STREAM_CASES + GEMV_CASES + GROUPED_CASES + DEEP_CASES + W4_CASES + GRAD_CASES
assert len({c.id for c in CASES}) == len(CASES)
FAMILIES = ("tiled", "splitk", "mid", "stream", "gemv", "grouped", "deep_k", "w4a16", "gradient")
assert {c.family for c in CASES} == set(FAMILIES)


def family(name):
    return [c for c in CASES if c.family == name]


# ---------------------------------------------------------------------------------------------------------------- inputs
# (A as a share of the default, c4 = 4 c, e): tried in order until the expected sum of |products|, with a 12 % margin, is below 2^24
LADDER = [(1.0, (4, 5, 6, 7), (6, 7, 8, 9)), (0.5, (4, 5, 6, 7), (6, 7, 8, 9)), (0.25, (4, 5, 6, 7), (6, 7, 8, 9)), (0.25, (4, 5), (8, 9))]
E_MAX = 9                    # the gradient's quantum: that of the smallest scale, 2^-(E_MAX + 4)


def level(case):
    """(A, c4 values, e values) for the case's shape: a function of (bits, op, reduction depth) alone."""
    base, mean_q = (4, 64.0) if case.bits == 8 else (64, 4.0)     # mean |q| over every code: 64 for int8, 4 for nibbles
    depth = case.N if case.op == "gemm_t" else case.K
    for share, c4s, es in LADDER:
        A = int(base * share)
        mean_i = A * (A + 1) / (2 * A + 1.0)                       # mean |i| of a uniform draw from -A .. A
        weight = np.mean(c4s) * np.mean([2.0 ** (E_MAX - e) for e in es]) if case.op == "gemm_t" else max(c4s)
        if depth * mean_i * mean_q * weight * 1.12 < LIMIT:
            return A, c4s, es
    raise AssertionError("no level of the ladder keeps %s below 2^24 quanta" % case.id)


class Weight:
    """q: int8 [K, N] codes (nibble values for int4); c4, e: int64 [N]; s = (c4 / 4) 2^-e as fp16"""

    def __init__(self, case, index=0):
        _, c4s, es = level(case)
        rng = np.random.default_rng([case.bits, case.K, case.N, int(case.op == "gemm_t"), index])
        lo, hi = (-128, 128) if case.bits == 8 else (-8, 8)
        self.q = rng.integers(lo, hi, size=(case.K, case.N), dtype=np.int8)
        self.c4 = rng.choice(np.array(c4s, np.int64), case.N)
        self.e = rng.choice(np.array(es, np.int64), case.N)
        self.s = (self.c4 / 4.0 * 2.0 ** -self.e).astype(np.float16)

    def dequant_f64(self):
        """q s in float64 (exact)"""
        return self.q.astype(np.float64) * self.s.astype(np.float64)[None, :]


def activations(case, index=0):
    """i: int8 [M, K] (gradient: [M, N]) uniform in -A .. A; x = i / 4 as fp16"""
    A = level(case)[0]
    rng = np.random.default_rng([case.bits, case.M, case.K, case.N, 7, index])
    cols = case.N if case.op == "gemm_t" else case.K
    return rng.integers(-A, A + 1, size=(case.M, cols), dtype=np.int8)


def as_x(i):
    return (i.astype(np.float32) / np.float32(4)).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------- reference
def int_sums(a, b):
    """a [R, D] . b [D, C] on integers held in float64 (exact: |sums| far below 2^53), in column blocks to bound the float64 copy of b"""
    a = np.ascontiguousarray(a, np.float64)
    out = np.empty((a.shape[0], b.shape[1]), np.float64)
    step = max(16, (1 << 25) // max(1, b.shape[0]))
    for c0 in range(0, b.shape[1], step):
        out[:, c0:c0 + step] = a @ b[:, c0:c0 + step].astype(np.float64, copy=False)
    return out


class Problem:
    """One product in quanta.  Forward: T[m, n] = c4[n] sum_k i[m, k] q[k, n], quantum[n] = 2^-(e[n] + 4).  Gradient:
    T[m, k] = sum_n i[m, n] g[n] q[k, n] with g = c4 2^(9 - e), quantum 2^-13.  Either way the reduction is i_w [R, D] . b [D, C]
    followed by a per-column factor, so the mutants below are written once."""

    def __init__(self, case, w, i, rows=None, cols=None):
        self.case = case
        i = i if rows is None else i[rows]
        if case.op == "gemm_t":
            assert cols is None
            g = w.c4 * 2 ** (E_MAX - w.e)
            self.a, b, self.col = i.astype(np.int64) * g[None, :], w.q.T, np.ones(case.K)
            self.quantum = np.full(case.K, 2.0 ** -(E_MAX + 4))
        else:
            cols = slice(None) if cols is None else cols          # a window of columns: the same sums, fewer of them
            self.a, b, self.col = i.astype(np.int64), w.q[:, cols], w.c4[cols].astype(np.float64)
            self.quantum = 2.0 ** -(w.e[cols] + 4.0)
        self.b = np.ascontiguousarray(b, np.float64) if b.size <= 1 << 25 else b    # (a large weight is converted block by block)
        self.D = self.a.shape[1]

    def sums(self, a=None, d0=0, d1=None):
        """T over the reduction range d0 .. d1 (the whole of it by default), in quanta"""
        a = self.a if a is None else a
        return int_sums(a[:, d0:d1], self.b[d0:d1]) * self.col[None, :]

    def bound(self):
        """sum |products| in quanta, per output element: THE CONDITION is bound().max() < LIMIT"""
        return int_sums(np.abs(self.a), np.abs(self.b) if self.b.dtype == np.float64 else np.abs(self.b.astype(np.int16))) * self.col[None, :]

    def f16(self, T):
        """quanta -> fp16, ONE rounding (float64 -> float16)"""
        return (T * self.quantum[None, :]).astype(np.float16)

    def f32(self, T):
        v = (T * self.quantum[None, :]).astype(np.float32)
        assert np.array_equal(v.astype(np.float64), T * self.quantum[None, :])       # below 2^24 quanta: an fp32 value
        return v

    def reference(self):
        return self.f16(self.sums())

    def term(self, d):
        """the products of reduction index d, in quanta: [R, C]"""
        return np.outer(self.a[:, d], self.b[d].astype(np.float64)) * self.col[None, :]

    def loud(self, d, step):
        """the reduction index nearest to d, walking by step, at which at least half of the rows have a non-zero activation (a lost
        product of a zero changes nothing: x = 0 is part of the inputs)"""
        while 2 * np.count_nonzero(self.a[:, d]) < self.a.shape[0]:
            d += step
        return d


def reference(case, w, i, rows=None):
    return Problem(case, w, i, rows).reference()


def quantum(case, w):
    """the quantum of every output column"""
    return np.full(case.K, 2.0 ** -(E_MAX + 4)) if case.op == "gemm_t" else 2.0 ** -(w.e + 4.0)


def quanta_between(case, w, got, want):
    """(got - want) in quanta of the column (fp16 values: the difference of the ROUNDED results)"""
    return (got.astype(np.float64) - want.astype(np.float64)) / quantum(case, w)[None, :]


# ---------------------------------------------------------------------------------------------------------------- mutants
def slice_bounds(D, S):
    """S slices of the reduction, cut at multiples of 64 (the k tile) as every sliced kernel cuts"""
    steps = D // 64
    return [64 * (steps * j // S) for j in range(S)] + [D]


def mutants(p):
    """{name: fp16 result of a kernel that breaks the contract in one way}, on Problem p.  Lost / doubled / shifted products keep fp32
    accumulation and one rounding; the fp16 mutants keep every product and round early."""
    T, D = p.sums(), p.D
    out = {"lost_first_k": p.f16(T - p.term(p.loud(0, 1))), "lost_last_k": p.f16(T - p.term(p.loud(D - 1, -1))),
           "lost_k_at_slice_seam": p.f16(T - p.term(p.loud(slice_bounds(D, 2)[1], 1))), "doubled_k": p.f16(T + p.term(p.loud(D // 3, 1)))}
    # the quietest product: the reduction index whose largest |product| over the rows and columns is smallest (the largest is
    # separable: max |a[:, d]| max |b[d] col|), among the indices at which at least half of the rows are non-zero.  What tier A makes
    # of ONE product depends on which one it is; this is the one it is most likely to accept.
    quiet = np.abs(p.a).max(0) * (np.abs(p.b if p.b.dtype == np.float64 else p.b.astype(np.float64)) * p.col[None, :]).max(1)
    quiet[2 * np.count_nonzero(p.a, axis=0) < p.a.shape[0]] = np.inf
    d = int(np.argmin(quiet))
    out["lost_quietest_k"], out["doubled_quietest_k"] = p.f16(T - p.term(d)), p.f16(T + p.term(d))
    out["x_shifted_by_one_k"] = p.f16(p.sums(np.roll(p.a, 1, axis=1)))
    tail = p.a.copy()                       # the last 8-element vector read one element over
    tail[:, D - 8:] = np.roll(p.a[:, D - 8:], -1, axis=1)
    out["last_vector_shifted_by_one_k"] = p.f16(T + p.sums(tail - p.a, D - 8, D))
    for S in (2, 4):
        if D // 64 >= S:
            b = slice_bounds(D, S)
            acc = np.zeros(T.shape, np.float32)
            for j in range(S):              # fp16(partial) of every slice, added in fp32
                acc = acc + p.f16(p.sums(None, b[j], b[j + 1])).astype(np.float32)
            out["fp16_partials_of_%d_slices" % S] = acc.astype(np.float16)
    if D >= 128:
        acc = np.zeros(T.shape, np.float16)
        for d0 in range(0, D, 64):          # the running accumulator parked in fp16 after every 64 k
            acc = (acc.astype(np.float32) + p.f32(p.sums(None, d0, min(D, d0 + 64)))).astype(np.float16)
        out["fp16_accumulator_every_64_k"] = acc
    return out


def differs(a, b):
    """share of elements that differ as numbers (-0 == +0)"""
    return float((a.astype(np.float32) != b.astype(np.float32)).mean())


# ---------------------------------------------------------------------------------------------------------------- sampling
def cpu_cols(case):
    """The columns the CPU checks take of a forward case: all of them up to 2^24 weights, else the first and the last ones."""
    if case.op == "gemm_t" or case.K * case.N <= 1 << 24:
        return None
    h = max(16, ((1 << 23) // case.K) // 16 * 16)
    return np.r_[0:h, case.N - h:case.N]


def cpu_rows(case, budget=5e7):
    """The rows the CPU checks (and the NumPy spot check of a device-side reference) take: all of them while rows x K x N stays within
    budget, else first / last / tile-seam rows, thinned to the budget (at least one)."""
    cols = cpu_cols(case)
    per_row = float(case.K) * (case.N if cols is None else len(cols))
    if case.M * per_row <= budget:
        return np.arange(case.M)
    rows = np.array(ac.sample_rows(case.M, 128 if case.M > 128 else 32))
    keep = max(1, min(len(rows), int(budget // per_row)))
    return rows[np.unique(np.linspace(0, len(rows) - 1, keep).round().astype(int))]


# ---------------------------------------------------------------------------------------------------------------- which kernel
def gemv_xv(form, M, K):
    """16-byte activation loads per thread of the staged GEMV forms (gemv.hip::launch_lds / launch_half): the power of two at or
    above ceil(M K / 8 / threads); the column units start at 2; 0 = activations in registers"""
    if form == "k4096_line" and M == 1:
        return 0
    threads = {"units8": 512, "units884": 512, "k4096_w8": 512, "generic8": 512, "shallow8": 512, "shallow4": 256, "shallow1": 64}.get(form, 1024)
    need = (M * K // 8 + threads - 1) // threads
    assert need <= 8, "no GEMV form stages this row"
    xv = 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8
    return max(xv, 2) if form.startswith("units") else xv


def gemv_form_i4(M, N, K, ncu=NCU):
    """gemv.hip::launch_m_i4 under the identity epilogue (no tuning overrides): (form, XV)"""
    KT, rows = K // 128, N // 16
    form = None
    if M == 1:
        pairs = KT % 2 == 0 and KT >= 32 and K <= 32768
        if pairs and ((KT != 64 and KT >= 40) or (KT not in (32, 64) and (2 * rows <= ncu or (rows > ncu and 10 * rows <= 13 * ncu)))):
            need = (K // 8 + 511) // 512
            return "units8", 2 if need <= 2 else 4 if need <= 4 else 8
        if KT == 32 and rows > 2 * ncu:
            form, threads = "k4096_w8", 512
    if form is None and M <= 2 and KT in (32, 64):
        return "line%d" % KT, 0
    if form is None:
        form, threads = (("generic16x4", 1024) if KT >= 64 else ("generic16x2", 1024) if KT >= 32 else ("shallow8", 512) if KT >= 16 else
                         ("shallow4", 256) if KT >= 4 else ("shallow1", 64))
    need = (M * K // 8 + threads - 1) // threads
    assert need <= 8 and M * K <= 65536, "no int4 GEMV form stages this row"
    return form, 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8


def grouped_bodies(K, N, count, ncu=NCU):
    """gemv.hip::launch_gemv_grouped for `count` problems of one shape: [(body, XV)] per dispatch of at most 32 problems"""
    assert K % 64 == 0 and K // 64 >= 32 and K <= 32768
    out = []
    for first in range(0, count, 32):
        rows = min(32, count - first) * (N // 16)
        if rows > 2 * ncu:
            need = (K // 8 + 511) // 512
            out.append(("w8", 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8))
        elif K == 4096:
            out.append(("w16_line", 1))
        else:
            need = (K // 8 + 1023) // 1024
            out.append(("w16", 1 if need <= 1 else 2 if need <= 2 else 4))
    return out


def tile_slices(M, N, K, ncu=NCU):
    """gemm.hip::tile_splitk_slices / wide_tile_splitk_slices under the identity epilogue: (K slices of the 128 x 64 tile, of the
    128 x 128 tile where the first is 1)"""
    rows, KT = (M + 127) // 128, K // 64
    narrow, wide = rows * ((N + 63) // 64), rows * ((N + 127) // 128)
    s1 = 4 if narrow * 4 <= ncu and KT // 4 >= 24 else 2 if narrow * 2 <= ncu and KT // 2 >= 40 else 1
    return s1, (2 if s1 == 1 and wide * 2 <= ncu and wide * 4 > ncu and KT // 2 >= 80 else 1)


def tile_plan(lib, bits, M, N, K, tile_j=0, cus=NCU):
    """eetq_diag_tile_plan under the identity epilogue: [(tile, first column or row, columns or rows, K slices)]"""
    rec = (ctypes.c_int * (6 * 64))(*([-9] * (6 * 64)))
    count = ctypes.c_int(-9)
    assert lib.eetq_diag_tile_plan(bits, M, N, K, 0, tile_j, cus, rec, 64, ctypes.byref(count)) == 0
    names = {2: "wide", 1: "narrow", 0: "stream"}
    out = []
    for n in range(count.value):
        r0, rows, c0, cols, tile, slices = rec[6 * n:6 * n + 6]
        out.append((names[tile], r0, rows, slices) if tile == 0 else (names[tile], c0, cols, slices))
    return out


def stream_plan(lib, bits, M, N, K):
    return ac._diag(lib, "eetq_diag_stream_plan", bits, M, N, K, NCU, outs=3)


def auto_path(lib, bits, M, N, K):
    return ac._diag(lib, "eetq_diag_auto_path", bits, M, N, K, outs=2)


def check_selection(lib, case):
    """The case's shape selects the form it is listed for UNDER THE IDENTITY EPILOGUE -- through the library's host queries where they
    exist, else through the restated launch arithmetic."""
    kind, want = case.select
    bits, M, N, K = case.bits, case.M, case.N, case.K
    if kind == "act":
        ac.check_selection(lib, want)                     # what the identity launch shares with the activated one, incl. eetq_diag_auto_path
        if want.select[0] == "mfma":                      # the identity launch of the tiled path: the same launches, K slices of its own
            slices = [2 if (want.id == "tile-ragged-round" and n == 1) else 1 for n in range(len(want.select[1]))]
            assert tile_plan(lib, 8, M, N, K) == [t + (s,) for t, s in zip(want.select[1], slices)], (case.id, tile_plan(lib, 8, M, N, K))
        if want.select[0] == "auto" and want.select[1][0] == TILESPLIT:     # the K-sliced tiled kernel: slices of the 128 x 64 tile
            assert tile_slices(M, N, K) == (want.select[1][1], 1), (case.id, tile_slices(M, N, K))
    elif kind == "tile_plan":
        assert tile_plan(lib, bits, M, N, K, want[0]) == want[1], (case.id, tile_plan(lib, bits, M, N, K, want[0]))
        if case.op == "tiled4":
            assert lib.eetq_w4a16_gemm_tiled_supported(M, N, K) == 1
    elif kind == "gemv_xv":
        form = ac.gemv_form(M, N, K)
        assert (form, gemv_xv(form, M, K)) == want, (case.id, form, gemv_xv(form, M, K))
        assert (case.path == "auto" and auto_path(lib, 8, M, N, K) == (GEMV, 0)) if M == 1 else (case.path == "gemv" and M <= 4), case.id
    elif kind == "gemv_i4":
        assert gemv_form_i4(M, N, K) == want, (case.id, gemv_form_i4(M, N, K))
        assert case.path == "gemv" or auto_path(lib, 4, M, N, K)[0] == GEMV, case.id
    elif kind == "stream":
        assert M <= 16 and case.path == "auto" and auto_path(lib, bits, M, N, K) == (STREAM, 0), (case.id, auto_path(lib, bits, M, N, K))
        assert stream_plan(lib, bits, M, N, K) == want, (case.id, stream_plan(lib, bits, M, N, K))
    elif kind == "stream_forced":
        assert M <= 16 and case.path == "stream" and stream_plan(lib, bits, M, N, K) == want, (case.id, stream_plan(lib, bits, M, N, K))
    elif kind == "stream_big":
        assert bits == 8 and case.path == "stream" and ac.stream_recipe_big(M, N, K) == want, case.id
    elif kind == "auto":
        assert bits == 8 and auto_path(lib, 8, M, N, K) == want, (case.id, auto_path(lib, 8, M, N, K))
        assert case.path == "auto" or (case.path == "tilesplit" and want[0] == TILESPLIT), case.id
        assert want[0] != TILESPLIT or tile_slices(M, N, K) == (want[1], 1), (case.id, tile_slices(M, N, K))   # slices of the narrow tile
    elif kind == "auto_wide":
        assert case.path == "auto" and M > 128 and auto_path(lib, 8, M, N, K) == want and tile_slices(M, N, K) == (1, 2), (case.id, tile_slices(M, N, K))
    elif kind == "auto_plan":
        assert case.path == "auto" and auto_path(lib, 8, M, N, K) == want[0] and ac.splitk_plan(lib, M, N, K) == want[1], (case.id, ac.splitk_plan(lib, M, N, K))
    elif kind == "auto_i4":
        assert case.path == "auto" and auto_path(lib, 4, M, N, K)[0] == want, case.id
    elif kind == "splitk_plan":
        nb, s, ring = want[:3]
        r = want[3] if len(want) > 3 else 1
        mt = (M + 32 * r - 1) // (32 * r)
        assert case.path == "splitk" and case.plan == ",".join(map(str, want)), case.id
        assert nb in (1, 2) and s in (1, 2, 4) and ring in (22, 33) and 1 <= mt <= 4 and (ring == 22 or mt <= 2) and r <= (32 if bits == 8 else 4), case.id
        assert (K // (64 if bits == 8 else 128) + 3) // 4 >= s, case.id     # no slice without a step: the plan runs as forced
        if r > 1:
            assert (M + 32 * mt - 1) // (32 * mt) == r, case.id
    elif kind == "expand":
        # the expansion route hands the int8 tile image to the W8A16 AUTO launch: AUTO for int4 at M > 128, path = "mfma" below
        assert bits == 4 and ((case.path == "auto" and auto_path(lib, 4, M, N, K)[0] == MFMA) or (case.path == "mfma" and M > 16)), case.id
        if want is not None:
            assert auto_path(lib, 8, M, N, K) == want, (case.id, auto_path(lib, 8, M, N, K))
    elif kind == "grouped":
        assert case.op == "grouped" and grouped_bodies(K, N, case.arg) == want, (case.id, grouped_bodies(K, N, case.arg))
    else:
        assert kind == "none" and (case.op == "gemm_t" or case.path == "mid"), case.id
