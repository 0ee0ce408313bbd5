"""Inputs, references and the table of cases of tests/test_gpu_act_epilogues.py: the bias + activation epilogue
y = fp16(act(acc + fp32(bias[n]))) [+ residual, an fp16 add] in every forward W8A16 kernel form that compiles it.  NumPy only, no GPU.

Two-hot rows.  Row m of x is zero except x[m, k1(m)] = x[m, k2(m)] = 1, so the fp32 accumulator of ANY kernel is exactly
a + b with a = wdq[k1, n], b = wdq[k2, n] (two fp16 values: their sum is exact in fp32, whatever the summation order or the K
slices), and the relu epilogue is computable bit for bit in float32.  k1 and k2 lie K/2 + 5 apart, i.e. in different quarters
of K: both K slices of a two-way split, and two of a four-way one, contribute.  tests/test_act_cases_cpu.py proves what the GPU
assertions rest on: the exactness, that every wrong order of the epilogue differs from the contract on >= 5 % of a case's
elements, and that each shape selects the kernel form it is listed for on an MI355X (256 CUs)."""
import ctypes
from collections import namedtuple

import numpy as np

NCU = 256                    # the chip the shapes are derived for
GEMV, MFMA, STREAM, MID, SPLITK, TILESPLIT = 1, 2, 3, 4, 5, 6
MUTANT_FLOOR = 0.05          # every mutant differs from the contract on at least this share of a case's elements
GELU_Z_MIN = -3.0            # below it 1 + tanh cancels: the calibrated gelu bound applies at z >= GELU_Z_MIN, tier A below
GELU_Z_SHARE = 0.90          # ... which holds at least this share of a case's elements

# path: the `path` argument of ops.w8_a16_gemm; plan: EETQ_AMD_SPLITK_PLAN for the launch (None: not set); form: the kernel form
# the case is meant to select, in words; select: what tests/test_act_cases_cpu.py checks it against (see check_selection)
Case = namedtuple("Case", "id M K N path plan form select twin seed")


def _case(id, M, K, N, path, form, select, plan=None, twin=None, seed=0):
    return Case(id, M, K, N, path, plan, form, select, twin, seed)


# ---------------------------------------------------------------------------------------------------------------- the cases
# Tiled kernel (gemm.hip::launch_gemm_mfma on 256 CUs; mfma_launches below restates its arithmetic)
TILED = [
    _case("tile-wide-act", 1000, 320, 4080, "mfma", "128 x 128 ACT tile: 256 wide / 512 narrow tiles; ragged last row tile, last column tile 112 wide",
          ("mfma", [("wide", 0, 4080)])),
    _case("tile-narrow-act", 200, 1024, 336, "mfma", "128 x 64 ACT tile, last column tile 16 wide", ("mfma", [("narrow", 0, 336)])),
    _case("tile-column-split", 640, 320, 6784, "mfma", "column split at c0 = 6528: wide ACT launch, then narrow ACT launch, every pointer moved",
          ("mfma", [("wide", 0, 6528), ("narrow", 6528, 256)]), twin="subproblem"),
    _case("tile-ragged-round", 1024, 5120, 5120, "mfma", "ragged round: two K slices under the identity epilogue, unsplit narrow ACT tiles with an activation",
          ("mfma", [("wide", 0, 4096), ("narrow", 4096, 1024)]), twin="subproblem"),
    _case("tile-shallow-k", 130, 256, 272, "mfma", "K < 320: stream kernel over 64-row chunks (64 + 64 + 2), residual pointer moving with the chunk",
          ("mfma", [("stream", 0, 64), ("stream", 64, 64), ("stream", 128, 2)])),
]
# Where act == 0 decides (abi.hip::auto_path_i8, gemm.hip::launch_gemm_tile_splitk)
ACT_GUARDS = [
    _case("guard-tilesplit-256", 256, 5120, 1024, "tilesplit", "identity: K in two slices; activated: tilesplit, AUTO and mfma are one kernel",
          ("auto", (TILESPLIT, 2)), twin="auto,mfma"),
    _case("guard-auto-128", 128, 8256, 1024, "auto", "identity AUTO: TILESPLIT with four slices; activated AUTO: the split-K plan",
          ("auto", (TILESPLIT, 4)), twin="splitk"),
]
# Split-K tile: K = 1088 (K % 256 != 0: five 256-deep steps), N = 272 (N % 32 != 0); plans forced as nb,s,ring[,r].
# MT = ceil(M / (32 r)) row blocks per workgroup: 17 -> 1, 50 -> 2, 80 -> 3, 100 / 128 -> 4 (ring 33 exists for MT <= 2)
SK_K, SK_N = 1088, 272
SPLITK_CASES = [_case("splitk-auto-17", 17, SK_K, SK_N, "auto", "AUTO at M = 17: the split-K tile on the planner's own plan", ("auto_path", SPLITK))]
for _M in (17, 50, 80, 100, 128):
    _plans = [(1, 1, 22), (2, 2, 22), (1, 4, 22)]
    if _M <= 64:
        _plans += [(2, 1, 33), (1, 2, 33)]
    if _M in (100, 128):
        _plans += [(2, 2, 22, 2), (1, 1, 33, 4)]
    for _p in _plans:
        SPLITK_CASES.append(_case("splitk-%d-%s" % (_M, "_".join(map(str, _p))), _M, SK_K, SK_N, "splitk",
                                  "split-K tile, %d-column blocks, %d K slice(s), ring %d, %d row group(s)" % (32 * _p[0], _p[1], _p[2], _p[3] if len(_p) > 3 else 1),
                                  ("splitk_plan", _p), plan=",".join(map(str, _p))))
MID_CASES = [_case("mid-33", 33, 1088, 272, "mid", "round-1 tile", ("none", None))]
# Stream kernel (streamk.hip::resolve): AUTO for M <= 16, path = "stream" above.  select = (form, tile rows per workgroup, waves) of
# eetq_diag_stream_plan at 256 CUs for M <= 16 (form 0 registers, 1 block copy, 2 ring); stream_recipe restates M > 16
STREAM_CASES = [
    _case("stream-ring8-w16", 5, 2048, 272, "auto", "8-row ring, 16 waves", ("stream", (2, 1, 16))),
    _case("stream-ring16-w16", 9, 2048, 272, "auto", "16-row ring, 16 waves", ("stream", (2, 1, 16))),
    _case("stream-ring16-w8-m12", 12, 2048, 272, "auto", "16-row ring, 8 waves", ("stream", (2, 1, 8))),
    _case("stream-ring16-w8-m16", 16, 2048, 272, "auto", "16-row ring, 8 waves", ("stream", (2, 1, 8))),
    _case("stream-ring32-m17", 17, 2048, 272, "stream", "32-row ring, one tile row per workgroup", ("stream_big", (2, 1, 8))),
    _case("stream-ring32-m32", 32, 2048, 272, "stream", "32-row ring, one tile row per workgroup", ("stream_big", (2, 1, 8))),
    _case("stream-regs-m40", 40, 2048, 272, "stream", "three row tiles, deep-K register form", ("stream_big", (0, 1, 16))),
    _case("stream-regs-nt2", 3, 2048, 4128, "auto", "registers, two tile rows, 8 waves", ("stream", (0, 2, 8))),
    _case("stream-ring32-nt2", 24, 2048, 4128, "stream", "32-row ring, two tile rows", ("stream_big", (2, 2, 8))),
    _case("stream-block-copy", 3, 2048, 8208, "auto", "block copy", ("stream", (1, 1, 8))),
    _case("stream-ring16-nt2", 12, 2048, 8224, "auto", "16-row ring, two tile rows", ("stream", (2, 2, 8))),
    _case("stream-ring8-nt2", 4, 2048, 12320, "auto", "8-row ring, two tile rows", ("stream", (2, 2, 8))),
    _case("stream-shallow-w1", 5, 64, 272, "auto", "one-wave shallow form", ("stream", (0, 1, 1))),
    _case("stream-shallow-w4", 5, 256, 272, "auto", "four-wave shallow form", ("stream", (0, 1, 4))),
]
# GEMV (gemv.hip::launch_m / half_units_pay / mixed_units_pay; gemv_form below restates them): M = 1 through AUTO, M = 2 .. 4 by path
GEMV_CASES = [
    # 17 tile rows: 2 * rows <= CUs, K / 64 = 32 even -> 8-column units (K / 256 = 8 < 16: not the mixed split)
    _case("gemv-units8", 1, 2048, 272, "auto", "8-column units", ("gemv", "units8")),
    # 8 + 8 + 4 needs half_units_pay (256 < rows <= 332) AND N % (4 * CUs) == 0 with N / CUs = 8a + 4 in 12 .. 28: N = 5120 is the only
    # width on 256 CUs (N = 3072 has 192 tile rows: neither few enough nor more than one per CU, it takes the straight-line form)
    _case("gemv-units884", 1, 4096, 5120, "auto", "8 + 8 + 4 column units", ("gemv", "units884")),
    # 129 tile rows: no units, <= 2 rows per CU -> 16 waves x 4 tiles, activations in registers
    _case("gemv-k4096-line", 1, 4096, 2064, "auto", "K = 4096 straight-line, 16 waves", ("gemv", "k4096_line")),
    # 513 tile rows > 2 per CU -> 8 waves, generic loop
    _case("gemv-k4096-w8", 1, 4096, 8208, "auto", "K = 4096, 8-wave generic form", ("gemv", "k4096_w8")),
    _case("gemv-generic-w16", 1, 2048, 2064, "auto", "16-wave generic form", ("gemv", "generic16")),
    _case("gemv-generic-w8", 1, 2048, 8208, "auto", "8-wave generic form", ("gemv", "generic8")),
    _case("gemv-shallow-1024", 1, 1024, 272, "auto", "shallow form, 8 waves", ("gemv", "shallow8")),
    _case("gemv-shallow-256", 1, 256, 272, "auto", "shallow form, 4 waves", ("gemv", "shallow4")),
    _case("gemv-shallow-64", 1, 64, 272, "auto", "shallow form, 1 wave", ("gemv", "shallow1")),
    # M = 2 .. 4: no units, no 8-wave forms, activations always through LDS
    _case("gemv-m3-k4096", 3, 4096, 2064, "gemv", "M = 3, K = 4096 straight-line through LDS", ("gemv", "k4096_line")),
    _case("gemv-m3-generic", 3, 2048, 2064, "gemv", "M = 3, 16-wave generic form", ("gemv", "generic16")),
    _case("gemv-m3-shallow", 3, 256, 272, "gemv", "M = 3, shallow form, 4 waves", ("gemv", "shallow4")),
    _case("gemv-m2-generic", 2, 2048, 272, "gemv", "M = 2, 16-wave generic form", ("gemv", "generic16")),
    _case("gemv-m4-shallow", 4, 1024, 272, "gemv", "M = 4, shallow form, 8 waves", ("gemv", "shallow8")),
]
CASES = TILED + ACT_GUARDS + SPLITK_CASES + MID_CASES + STREAM_CASES + GEMV_CASES
assert len({c.id for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------- inputs
def weight(K, N):
    """Random int8 weight with every code -128 .. 127 and fp16 scales in [1e-3, 2.1e-2] (as tests/test_gpu_gemm_t.py::_weight)."""
    rng = np.random.default_rng(K * 7 + N)
    q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    s = (rng.random(N, dtype=np.float32) * 0.02 + 1e-3).astype(np.float16)
    return q, s


def hot_columns(M, K):
    """k1(m), k2(m): K/2 + 5 apart (mod K), so never in the same quarter of K."""
    m = np.arange(M, dtype=np.int64)
    return (37 * m) % K, (37 * m + K // 2 + 5) % K


def two_hot_x(M, K):
    x = np.zeros((M, K), np.float16)
    k1, k2 = hot_columns(M, K)
    x[np.arange(M), k1] = 1
    x[np.arange(M), k2] = 1
    return x


def bias_residual(case):
    """fp16 bias ~ N(0, 0.5) and residual ~ N(0, 1)."""
    rng = np.random.default_rng([case.M, case.K, case.N, case.seed])
    bias = (rng.standard_normal(case.N) * 0.5).astype(np.float16)
    res = rng.standard_normal((case.M, case.N)).astype(np.float16)
    return bias, res


def random_x(case):
    """Both signs, as test_gpu_parity.py::test_activation_epilogues_vs_oracle builds it."""
    rng = np.random.default_rng([case.M, case.K, case.N, case.seed, 1])
    return (rng.random((case.M, case.K)) - 0.5).astype(np.float16)


def hot_weights(oracle, q, s, M):
    """a[m, n], b[m, n]: the two dequantised weights row m multiplies by one (fp16, oracle.dequant)."""
    k1, k2 = hot_columns(M, q.shape[0])
    return oracle.dequant(np.ascontiguousarray(q[k1]), s), oracle.dequant(np.ascontiguousarray(q[k2]), s)


# ---------------------------------------------------------------------------------------------------------------- references
def acc_f32(a, b):
    """The accumulator: one fp32 add of two fp16 values."""
    return a.astype(np.float32) + b.astype(np.float32)


def z_f32(a, b, bias):
    """acc + fp32(bias): one more fp32 add, as finish_element / finish_quad do it."""
    acc = acc_f32(a, b)
    return acc if bias is None else acc + bias.astype(np.float32)[None, :]


def relu_contract(a, b, bias, res=None):
    want = np.maximum(z_f32(a, b, bias), np.float32(0)).astype(np.float16)
    return want if res is None else want + res          # the residual: a second add, in float16


def relu_mutants(a, b, bias, res):
    """Wrong epilogues, each with the contract's result it has to be told apart from: {name: (mutant, contract)}."""
    acc, b32, zero = acc_f32(a, b), bias.astype(np.float32), np.float32(0)
    want, want_res = relu_contract(a, b, bias), relu_contract(a, b, bias, res)
    out = {"round_then_add": (np.maximum(acc.astype(np.float16).astype(np.float32) + b32[None, :], zero).astype(np.float16), want),
           "residual_before_act": (np.maximum(acc + b32[None, :] + res.astype(np.float32), zero).astype(np.float16), want_res),
           "identity": ((acc + b32[None, :]).astype(np.float16), want)}
    for shift in (1, 8, 16, 64):
        out["bias_column_plus_%d" % shift] = (np.maximum(acc + np.roll(b32, -shift)[None, :], zero).astype(np.float16), want)
    if a.shape[0] > 1:                                   # (a single row has no next row)
        out["row_to_next_row"] = (np.roll(want, 1, axis=0), want)
    return out


def act_f64(z, act):
    """The oracle's formula (oracle_w8a16_gemm_bias_act): evaluated in double on the fp32 z, rounded to fp32, then fp16."""
    z = z.astype(np.float64)
    if act == "relu":
        r = np.maximum(z, 0.0)
    elif act == "silu":
        r = z / (1.0 + np.exp(-z))
    else:
        r = 0.5 * z * (1.0 + np.tanh(0.7978845608028654 * z * (1.0 + 0.044715 * z * z)))
    return r.astype(np.float32).astype(np.float16)


def act_f32(z, act):
    """The same formula with every operation in float32 (the device's order of operations, NumPy's expf / tanhf)."""
    z, one = z.astype(np.float32), np.float32(1)
    if act == "relu":
        r = np.maximum(z, np.float32(0))
    elif act == "silu":
        r = z / (one + np.exp(-z))
    else:
        r = np.float32(0.5) * z * (one + np.tanh(np.float32(0.7978845608028654) * z * (one + np.float32(0.044715) * z * z)))
    assert r.dtype == np.float32
    return r.astype(np.float16)


def f16_ordinal(h):
    """fp16 -> an integer that counts representable values in order; -0 and +0 both map to 0."""
    bits = np.ascontiguousarray(h, np.float16).view(np.uint16).astype(np.int32)
    mag = bits & 0x7FFF
    return np.where(bits & 0x8000, -mag, mag)


def ulp_distance(x, y):
    return np.abs(f16_ordinal(x) - f16_ordinal(y))


def calibrated_allowance(z, act):
    """Per element, in fp16 ulps: the distance between the float32 and the double evaluation of the formula at that z, plus one --
    from the two references alone.  Returns (allowance, the double reference as fp16)."""
    ref = act_f64(z, act)
    return ulp_distance(act_f32(z, act), ref) + 1, ref


def tier_a(y, ref):
    y, ref = np.asarray(y, np.float32), np.asarray(ref, np.float32)
    return np.abs(y - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)


def check_calibrated(got, z, act):
    """The device's silu / gelu on the two-hot rows against calibrated_allowance; gelu below GELU_Z_MIN against tier A.
    Returns (ok mask, largest distance among the calibrated elements, share of calibrated elements that differ from the reference)."""
    allow, ref = calibrated_allowance(z, act)
    dist = ulp_distance(got, ref)
    cal = np.ones(z.shape, bool) if act != "gelu" else z >= np.float32(GELU_Z_MIN)
    ok = np.where(cal, dist <= allow, tier_a(got, ref))
    return ok, int(dist[cal].max()), float((dist[cal] > 0).mean())


# ---------------------------------------------------------------------------------------------------------------- sampling
def row_group(case):
    """Rows per row tile / row group of the kernel the case runs."""
    if case.path == "splitk" and case.plan:
        p = [int(v) for v in case.plan.split(",")]
        r = p[3] if len(p) > 3 else 1
        return 32 * ((case.M + 32 * r - 1) // (32 * r))
    if case.select[0] == "mfma" and case.select[1][0][0] == "stream":
        return 64                                        # K < 320: 64-row chunks of the stream kernel
    return 128 if case.path in ("mfma", "tilesplit") else 32   # (32: every row block a split-K plan or the round-1 tile can cut)


def sample_rows(M, group):
    """All rows up to M = 64; above, {0, 31, 32, M/2, M-1} and the first and last row of every row tile or group."""
    if M <= 64:
        return list(range(M))
    rows = {0, 31, 32, M // 2, M - 1}
    for g0 in range(0, M, group):
        rows |= {g0, min(g0 + group, M) - 1}
    return sorted(r for r in rows if 0 <= r < M)


def sample_columns(rows, K, N, seams=()):
    """Every column while the oracle's rows x K x N products stay below 1.5e8; else 96-column windows at both ends, the middle and
    either side of every seam (a column where one launch ends and the next begins)."""
    if rows * K * N <= 150e6:
        return np.arange(N)
    cols = set(range(96)) | set(range(N - 96, N)) | set(range(N // 2 - 48, N // 2 + 48))
    for c0 in seams:
        cols |= set(range(c0 - 96, c0 + 96))
    return np.array(sorted(c for c in cols if 0 <= c < N))


# ---------------------------------------------------------------------------------------------------------------- which kernel
def mfma_launches(M, N, K, ncu=NCU):
    """gemm.hip::launch_gemm_mfma with an activation: [(tile, first column or row, columns or rows)], tile = wide (128 x 128),
    narrow (128 x 64) or stream (K < 320: the stream kernel over 64-row chunks).  (M * K * 2 < 2^31: one row chunk.)"""
    if K // 64 < 5:
        return [("stream", m, min(64, M - m)) for m in range(0, M, 64)]
    tiles_m = (M + 127) // 128

    def cols(c0, n, force):
        t2, t1 = tiles_m * ((n + 127) // 128), tiles_m * ((n + 63) // 64)
        narrow = force == 1 or (force == 0 and 0.70 * ((t1 + ncu - 1) // ncu) < ((t2 + ncu - 1) // ncu))
        return ("narrow" if narrow else "wide", c0, n)

    T2 = tiles_m * ((N + 127) // 128)
    rem = T2 % ncu
    if T2 > ncu and rem != 0 and rem * 2 < ncu and tiles_m <= ncu:
        cols1 = ((T2 - rem) // tiles_m) * 128
        if 0 < cols1 < N:
            return [cols(0, cols1, 2), cols(cols1, N - cols1, 0)]   # (an activated ragged round is never K-sliced: act != 0)
    return [cols(0, N, 0)]


def ragged_round_slices(M, N, K, ncu=NCU):
    """K slices of the ragged round under the IDENTITY epilogue (gemm.hip: launch_tile_splitk_cols): 2 or 1."""
    tiles_m = (M + 127) // 128
    T2 = tiles_m * ((N + 127) // 128)
    rem = T2 % ncu
    if not (T2 > ncu and rem != 0 and rem * 2 < ncu):
        return 1
    cols1 = ((T2 - rem) // tiles_m) * 128
    rem_tiles = tiles_m * ((N - cols1 + 63) // 64)
    return 2 if rem_tiles * 2 <= ncu and (K // 64) // 2 >= 40 else 1


def gemv_form(M, N, K, ncu=NCU):
    """gemv.hip::launch_m with an activation epilogue (no prologue, no tuning overrides)."""
    KT, rows = K // 64, N // 16
    if M == 1:
        half = KT % 2 == 0 and KT >= 32 and K <= 32768 and (2 * rows <= ncu or (rows > ncu and 10 * rows <= 13 * ncu))
        if half:
            per = N // ncu
            mixed = KT % 4 == 0 and KT // 4 >= 16 and N % (4 * ncu) == 0 and per % 8 == 4 and 12 <= per <= 28
            return "units884" if mixed else "units8"
        if KT == 64 and rows > 2 * ncu:
            return "k4096_w8"
    if KT == 64:
        return "k4096_line"
    if M == 1 and KT >= 32 and K <= 32768 and rows > 2 * ncu:
        return "generic8"
    return "generic16" if KT >= 32 else "shallow8" if KT >= 16 else "shallow4" if KT >= 4 else "shallow1"


def stream_recipe_big(M, N, K, ncu=NCU):
    """streamk.hip::resolve for 17 <= M <= 64 at K / 64 >= 32 (no overrides): (form, tile rows per workgroup, waves)."""
    assert 16 < M <= 64 and K // 64 >= 32
    if (M + 15) // 16 > 2:
        return (0, 1, 16)
    nt = 1 if N // 16 <= ncu else 2
    return (2, nt if N % 32 == 0 else 1, 8)


def _diag(lib, name, *args, outs):
    vals = [ctypes.c_int(-9) for _ in range(outs)]
    assert getattr(lib, name)(*args, *[ctypes.byref(v) for v in vals]) == 0, name
    return tuple(v.value for v in vals)


def auto_path(lib, M, N, K):
    """(EETQ_PATH_*, detail) of the IDENTITY launch (eetq_diag_auto_path; without a device the rule is the 256-CU chip's)."""
    return _diag(lib, "eetq_diag_auto_path", 8, M, N, K, outs=2)


def splitk_plan(lib, M, N, K):
    """(column blocks, K slices, ring, row groups) the split-K tile runs the shape with (eetq_diag_splitk_plan, 256 CUs)."""
    return _diag(lib, "eetq_diag_splitk_plan", M, N, K, outs=4)


# the plan an ACTIVATED AUTO launch runs where the table sends one to the split-K tile: at M = 128 a combination no forced plan of
# the table has (K slices AND row groups on the 3-deep ring)
ACTIVATED_PLAN = {"splitk-auto-17": (1, 1, 33, 1), "guard-auto-128": (2, 4, 33, 4)}


def check_selection(lib, case):
    """The case's shape selects the form it is listed for -- through the library's host queries where they exist, else through the
    restatements above."""
    kind, want = case.select
    M, N, K = case.M, case.N, case.K
    if kind == "mfma":
        assert mfma_launches(M, N, K) == want, (case.id, mfma_launches(M, N, K))
        if case.id == "tile-ragged-round":
            assert ragged_round_slices(M, N, K) == 2
    elif kind == "auto":
        assert auto_path(lib, M, N, K) == want, (case.id, auto_path(lib, M, N, K))
        if case.id in ACTIVATED_PLAN:            # activated AUTO at 97 <= M <= 128: act != 0 skips the K-sliced tiled kernel
            assert splitk_plan(lib, M, N, K) == ACTIVATED_PLAN[case.id], (case.id, splitk_plan(lib, M, N, K))
        if case.path == "tilesplit":             # activated: launch_gemm_tile_splitk -> launch_gemm_mfma, the narrow ACT tile
            assert mfma_launches(M, N, K) == [("narrow", 0, N)]
    elif kind == "auto_path":
        assert auto_path(lib, M, N, K)[0] == want, case.id
        assert splitk_plan(lib, M, N, K) == ACTIVATED_PLAN[case.id], (case.id, splitk_plan(lib, M, N, K))
    elif kind == "splitk_plan":
        nb, s, ring = want[:3]
        r = want[3] if len(want) > 3 else 1
        mt = (M + 32 * r - 1) // (32 * r)
        assert nb in (1, 2) and s in (1, 2, 4) and ring in (22, 33) and 1 <= mt <= 4 and (ring == 22 or mt <= 2), case.id
        assert (K // 64 + 3) // 4 >= s, case.id       # no slice without a 256-deep step: the plan runs as forced
        if r > 1:
            assert (M + 32 * mt - 1) // (32 * mt) == r, case.id   # launch_full derives the group count back from MT
    elif kind == "stream":
        assert M <= 16 and auto_path(lib, M, N, K) == (STREAM, 0), case.id
        assert _diag(lib, "eetq_diag_stream_plan", 8, M, N, K, NCU, outs=3) == want, case.id
    elif kind == "stream_big":
        assert case.path == "stream" and stream_recipe_big(M, N, K) == want, case.id
    elif kind == "gemv":
        assert gemv_form(M, N, K) == want, (case.id, gemv_form(M, N, K))
        if M == 1:
            assert case.path == "auto" and auto_path(lib, M, N, K) == (GEMV, 0), case.id
        else:
            assert case.path == "gemv" and M <= 4
    else:
        assert kind == "none"
