"""Reduction depths 16384 < K <= 65536 (and just past them): the down projections of Mixtral-8x22B (16384), Llama-2/3-70B (28672) and
Llama-3.1-405B (53248).  Above K = 16384 the launchers take decisions no other test reaches: eight 16-byte activation loads per thread
(XV = 8) in every GEMV form, LDS staging beyond 64 KiB, the K cut-offs of the column-unit and grouped kernels, the hard limits of LDS
staging, 100+ K steps per slice of the split plans, and the second trip of the quantiser's loop over 32 row-block maxima.

Weights are random integer codes drawn on the GPU (every int8 code / every nibble) with fp16 scales, packed by
ops.preprocess_weights (bit-exact elsewhere: test_gpu_parity.py, test_gpu_int4.py).  Two references, both at tier A,
|err| <= 1e-3 * max|y| + 2e-3 * |y|:
  (a) the oracle (exact accumulation) on sampled columns: the first 48, the last 48 and 160 random ones;
  (b) on every element, torch's fp32 product of the activations with the fp16-dequantised weight, in column chunks on the GPU.
Activations are uniform in [0, 1) with every second or third column negated.  The comment by each shape says which instantiation it
reaches on a 256-CU MI355X and why; where a host-side diagnostic names the decision it is asserted, so a change of rule fails here
instead of moving the test off its target."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEMV, MFMA, STREAM, MID, SPLITK, TILESPLIT = 1, 2, 3, 4, 5, 6
REGS, BLOCK, RING = 0, 1, 2
STAGING = "too large for LDS staging"


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as _ops
    from eetq_amd import _lib
    assert _lib.lib().eetq_device_supported() == 1, "kernels are built for gfx950 only"
    assert torch.cuda.get_device_properties(0).multi_processor_count == 256, "the shapes below are derived for 256 CUs"
    return _ops


def _auto(bits, M, N, K):
    from eetq_amd import _lib
    p, d = ctypes.c_int(-9), ctypes.c_int(-9)
    _lib.check(_lib.lib().eetq_diag_auto_path(bits, M, N, K, ctypes.byref(p), ctypes.byref(d)))
    return p.value, d.value


def _stream_plan(bits, M, N, K):
    from eetq_amd import _lib
    f, t, w = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_int(-9)
    assert _lib.lib().eetq_diag_stream_plan(bits, M, N, K, 0, ctypes.byref(f), ctypes.byref(t), ctypes.byref(w)) == 0
    return f.value, t.value, w.value


def _sample_cols(N):
    if N <= 512:
        return np.arange(N)
    return np.unique(np.concatenate([np.arange(48), np.arange(N - 48, N), np.random.default_rng(N).integers(0, N, 160)]))


def _i4_values(raw):
    """packed int4 bytes [K, N/2] -> the values -8 .. 7 as int8 [K, N]: column 2j is the low nibble (oracle.i4_values)"""
    b = raw.short()
    return torch.stack([((b & 15) ^ 8) - 8, b >> 4], dim=2).reshape(raw.shape[0], -1).to(torch.int8)


class _Case:
    """One weight with its activations and references, built once and shared by every test case on that (bits, K, N)."""

    def __init__(self, ops, oracle, bits, K, N, rows, oracle_rows, negate):
        g = torch.Generator(device=DEV)
        g.manual_seed(K * 7 + N + bits)
        self.bits, self.K, self.N = bits, K, N
        if bits == 8:
            self.q = torch.randint(-128, 128, (K, N), dtype=torch.int8, device=DEV, generator=g)
            self.packed = ops.preprocess_weights(self.q)
        else:
            raw = torch.randint(-128, 128, (K, N // 2), dtype=torch.int8, device=DEV, generator=g)
            self.q = _i4_values(raw)
            self.packed = ops.preprocess_weights(raw, True)
            del raw
        self.s = (torch.rand(N, device=DEV, generator=g) * 0.02 + 1e-3).half()
        self.x = torch.rand(rows, K, device=DEV, generator=g).half()
        self.x[:, ::negate] *= -1
        # (b): fp32 product with the fp16-dequantised weight (q.half() * s is fp16(q * s): the product is exact in fp32)
        self.ref = torch.empty(rows, N, dtype=torch.float32, device=DEV)
        xf = self.x.float()
        step = max(16, min(N, (32 << 20) // K))
        for c0 in range(0, N, step):
            c1 = min(N, c0 + step)
            self.ref[:, c0:c1] = xf @ (self.q[:, c0:c1].half() * self.s[None, c0:c1]).float()
        del xf
        # (a): the oracle on sampled columns of a few rows
        self.cols = _sample_cols(N)
        ct = torch.from_numpy(self.cols).to(DEV)
        self.orows = sorted(r for r in set(oracle_rows) if r < rows)
        self.q_cols = np.ascontiguousarray(self.q[:, ct].cpu().numpy())
        self.s_cols = np.ascontiguousarray(self.s[ct].cpu().numpy())
        self.cols_t = ct
        self.oref = {}
        if self.orows:
            o = oracle.w8a16_gemm(self.x[self.orows].cpu().numpy(), self.q_cols, self.s_cols).astype(np.float32)
            self.oref = {r: o[i] for i, r in enumerate(self.orows)}
        self._oracle = oracle

    def check(self, y, M, what):
        assert y.shape == (M, self.N) and y.dtype == torch.float16, what
        ref = self.ref[:M]
        err = (y.float() - ref).abs()
        bad = err > 1e-3 * ref.abs().max() + 2e-3 * ref.abs()
        assert not bool(bad.any()), (what, "fp32 reference", int(bad.sum()), float(err.max()), torch.nonzero(bad)[:4].tolist())
        rows = [r for r in self.orows if r < M]
        if rows:
            got = y[rows][:, self.cols_t].float().cpu().numpy()
            o = np.stack([self.oref[r] for r in rows])
            tol = 1e-3 * np.abs(o).max() + 2e-3 * np.abs(o)
            assert np.all(np.abs(got - o) <= tol), (what, "oracle", float(np.abs(got - o).max()))


_cases = {}


def _case(ops, oracle, bits, K, N, rows=1, oracle_rows=(0,), negate=3):
    key = (bits, K, N, rows, tuple(oracle_rows), negate)
    if key not in _cases:
        _cases.clear()   # one weight at a time: the largest is half a gigabyte
        torch.cuda.empty_cache()
        _cases[key] = _Case(ops, oracle, bits, K, N, rows, oracle_rows, negate)
    return _cases[key]


def _epilogue(ops, c, M, y, **kw):
    """fused bias + residual == the separate fp16 adds, bit for bit"""
    g = torch.Generator(device=DEV)
    g.manual_seed(M + c.N)
    bias = torch.randn(c.N, device=DEV, generator=g).half()
    res = torch.randn(M, c.N, device=DEV, generator=g).half()
    fused = ops.w8_a16_gemm(c.x[:M], c.packed, c.s, bias=bias, residual=res, **kw)
    assert torch.equal(fused, (y + bias) + res), kw


# ---------------------------------------------------------------------------------------------- int8, M = 1

# 256 CUs.  rows = N / 16 tile rows; "need" = 16-byte activation loads per thread = ceil(K / 8 / threads) -> XV = 1 / 2 / 4 / 8.
# Column units (gemv.hip::half_units_pay): K / 64 even, K <= 32768 and rows <= 128 or 256 < rows <= 332; 8 waves = 512 threads.
M1_SHAPES = [
    # K = 28672 (K / 64 = 448), rows = 4 <= 128: 8-column units, need = ceil(3584 / 512) = 7 -> gemv_half_kernel<8, 2, XV = 8>
    (28672, 64, True),
    # rows = 320, N = 20 columns per CU = 8 + 8 + 4 (mixed_units_pay: N % 1024 == 0, N / 256 % 8 == 4): gemv_mixed_kernel<8, 2, XV = 8>.
    # (N = 3072, rows = 192, is neither <= 128 nor > 256: it takes the generic 16-wave form; 5120 is the one N with this split.)
    (28672, 5120, True),
    # K / 64 = 449 is odd: no units; rows = 4 <= 512: 16 waves = 1024 threads, need = ceil(3592 / 1024) = 4 -> gemv_kernel<1, 16, 2, .., XV = 4>
    (28736, 64, True),
    # rows = 513 > 2 * 256 and > 332: the 8-wave generic form, need = 7 -> gemv_kernel<1, 8, 2, false, false, XV = 8, 8>
    (28672, 8208, True),
    # K > 32768: no units; 16 waves, need = ceil(6656 / 1024) = 7 -> XV = 8; 104 KiB of activations + 1 KiB: the large-LDS opt-in
    (53248, 64, True),
    # the last K the GEMV stages: need = 8192 / 1024 = 8, 129 KiB of LDS
    (65536, 64, True),
    # rows = 513 > 2 * 256 with K > 32768: the 8-wave form cannot stage the row (need = 9 and 13); the 16-wave form runs (XV = 8)
    (32832, 8208, True),
    (53248, 8208, True),
    # past the limit of every GEMV form (need = 9 with 16 waves): AUTO runs the small-batch kernel with one row
    (65600, 64, False),
]


@pytest.mark.parametrize("K,N,staged", M1_SHAPES)
def test_m1_int8_forms_above_k_16384(ops, oracle, K, N, staged):
    c = _case(ops, oracle, 8, K, N, negate=2 if N == 64 else 3)
    assert _auto(8, 1, N, K) == ((GEMV if staged else STREAM), 0)
    y = ops.w8_a16_gemm(c.x, c.packed, c.s)
    c.check(y, 1, "auto")
    assert torch.equal(y, ops.w8_a16_gemm(c.x, c.packed, c.s))
    _epilogue(ops, c, 1, y)
    if staged:
        forced = ops.w8_a16_gemm(c.x, c.packed, c.s, path="gemv")
        assert torch.equal(forced, y)            # AUTO is this launch
        _epilogue(ops, c, 1, forced, path="gemv")
    else:
        with pytest.raises(RuntimeError, match=STAGING):
            ops.w8_a16_gemm(c.x, c.packed, c.s, path="gemv")
        assert torch.equal(ops.w8_a16_gemm(c.x, c.packed, c.s, path="stream"), y)


# K = 28672: the 8-column units with the prologue (gemv_half_kernel<8, 2, XV = 8, 8, NORM = 1 / 2>); K = 53248: the 16-wave form
# (gemv_kernel<1, 16, 2, false, false, XV = 8, 8, NORM = 1 / 2>, 105 KiB of LDS)
@pytest.mark.parametrize("K,N", [(28672, 64), (53248, 64)])
def test_m1_rmsnorm_prologue(ops, oracle, K, N):
    """test_gemv_rmsnorm_prologue's assertions: the fused norm may differ from the separate one by an fp16 ulp in rare elements"""
    c = _case(ops, oracle, 8, K, N, negate=2)
    xd = c.x * 3.0
    g = torch.Generator(device=DEV)
    g.manual_seed(K)
    gamma = (torch.rand(K, device=DEV, generator=g) + 0.5).half()
    eps = 1e-5
    normed = torch.empty_like(xd)
    ops.layernorm_forward(xd, gamma, normed, eps)
    sep = ops.w8_a16_gemm(normed, c.packed, c.s)
    fused = ops.w8_a16_gemm(xd, c.packed, c.s, norm=(gamma, eps))
    assert (fused.float() - sep.float()).abs().max().item() <= 2e-3 * sep.float().abs().max().item() + 1e-4
    xn = oracle.rmsnorm_f16(xd.cpu().numpy(), gamma.cpu().numpy(), eps)
    ref = oracle.w8a16_gemm(xn, c.q.cpu().numpy(), c.s.cpu().numpy()).astype(np.float32)
    assert np.all(np.abs(fused.cpu().numpy().astype(np.float32) - ref) <= 2e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref))
    bias = torch.randn(N, device=DEV, generator=g).half()
    res = torch.randn(1, N, device=DEV, generator=g).half()
    assert torch.equal(ops.w8_a16_gemm(xd, c.packed, c.s, norm=(gamma, eps), bias=bias, residual=res), res + (fused + bias))


@pytest.mark.parametrize("K,N", [(28672, 64), (53248, 64)])
def test_m1_gated_prologue(ops, oracle, K, N):
    """test_gemv_gated_activation_prologue's assertions: the same roundings as silu_mul + GEMV, so bit-identical"""
    c = _case(ops, oracle, 8, K, N, negate=2)
    g = torch.Generator(device=DEV)
    g.manual_seed(K)
    gu = (torch.randn(1, 2 * K, device=DEV, generator=g) * 2).half()
    act = ops.silu_mul(gu)
    sep = ops.w8_a16_gemm(act, c.packed, c.s)
    fused = ops.w8_a16_gemm(gu, c.packed, c.s, gated=True)
    assert torch.equal(fused, sep)
    ref = oracle.w8a16_gemm(act.cpu().numpy(), c.q.cpu().numpy(), c.s.cpu().numpy()).astype(np.float32)
    assert np.all(np.abs(fused.cpu().numpy().astype(np.float32) - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref))
    bias = torch.randn(N, device=DEV, generator=g).half()
    res = torch.randn(1, N, device=DEV, generator=g).half()
    assert torch.equal(ops.w8_a16_gemm(gu, c.packed, c.s, gated=True, bias=bias, residual=res), res + (sep + bias))


@pytest.mark.parametrize("binding", ["ops", "ops_ctypes"])
def test_m1_fused_prologues_fall_back_to_the_unfused_sequence_past_the_staging_limit(ops, oracle, binding):
    """K = 65600: no GEMV form stages the row, so the fused M = 1 entry points refuse it and the operator runs norm / silu_mul and
    the projection as separate launches -- bit for bit the sequence a caller would write."""
    import importlib
    from eetq_amd import _lib
    b = importlib.import_module("eetq_amd." + binding)
    K, N = 65600, 64
    c = _case(ops, oracle, 8, K, N, negate=2)
    g = torch.Generator(device=DEV)
    g.manual_seed(K)
    gamma = (torch.rand(K, device=DEV, generator=g) + 0.5).half()
    bias = torch.randn(N, device=DEV, generator=g).half()
    res = torch.randn(1, N, device=DEV, generator=g).half()
    gu = (torch.randn(1, 2 * K, device=DEV, generator=g) * 2).half()
    eps = 1e-5
    xd = c.x * 3.0
    normed = torch.empty_like(xd)
    b.layernorm_forward(xd, gamma, normed, eps)
    assert torch.equal(b.w8_a16_gemm(xd, c.packed, c.s, norm=(gamma, eps), bias=bias, residual=res),
                       b.w8_a16_gemm(normed, c.packed, c.s, bias=bias, residual=res))
    assert torch.equal(b.w8_a16_gemm(gu, c.packed, c.s, gated=True, bias=bias, residual=res),
                       b.w8_a16_gemm(b.silu_mul(gu), c.packed, c.s, bias=bias, residual=res))
    for norm, xin in ((None, xd), ((gamma, eps), normed)):
        assert torch.equal(b.w8_a16_gemm(xd, c.packed, c.s, bias=bias, norm=norm, activation="silu_glu8"),
                           b.silu_mul(b.w8_a16_gemm(xin, c.packed, c.s, bias=bias), True))
    c.check(b.w8_a16_gemm(c.x, c.packed, c.s), 1, binding)
    # the entry points themselves keep refusing, with the staging message and nothing written
    L = _lib.lib()
    y = torch.full((1, N), 7.0, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rc in (L.eetq_w8a16_gemv_rmsnorm(p(xd), p(gamma), eps, p(c.packed), p(c.s), None, None, p(y), N, K, st),
               L.eetq_w8a16_gemv_silu_gated(p(gu), p(c.packed), p(c.s), None, None, p(y), N, K, st),
               L.eetq_w8a16_gemv_glu8(p(xd), None, 0.0, p(c.packed), p(c.s), None, p(y), N, K, st)):
        assert rc == _lib.ERR_UNSUPPORTED and STAGING.encode() in L.eetq_last_error()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ---------------------------------------------------------------------------------------------- int8, M = 2 .. 4 on the GEMV

def _gemv_into(x, c, y):
    from eetq_amd import ops_ctypes
    return ops_ctypes._gemm_launch(x, c.packed, c.s, y, x.shape[0], c.N, c.K, ops_ctypes._PATHS["gemv"])


# launch_m<M>, K / 64 >= 32: 16 waves x 2 tiles, 1024 threads; need = ceil(M * K / 8 / 1024)
@pytest.mark.parametrize("M,K", [(2, 28672),    # need = 7 -> XV = 8, 114 KiB of LDS
                                 (3, 21760),    # need = ceil(7.97) = 8, 130.5 KiB
                                 (4, 16384)])   # need = 8 exactly, 132 KiB: the most rows x depth the GEMV stages
def test_gemv_m2_to_4_inside_the_staging_limit(ops, oracle, M, K):
    c = _case(ops, oracle, 8, K, 64, rows=M, oracle_rows=(0, M - 1), negate=2)
    y = ops.w8_a16_gemm(c.x, c.packed, c.s, path="gemv")
    c.check(y, M, "gemv")
    _epilogue(ops, c, M, y, path="gemv")
    c.check(ops.w8_a16_gemm(c.x, c.packed, c.s), M, "auto")


@pytest.mark.parametrize("M,K", [(4, 16448),    # need = ceil(8224 / 1024) = 9: no instantiation loads that many
                                 (4, 20480)])   # 160 KiB of activations + 4 KiB of partial sums: over the 160 KiB of a CU
def test_gemv_m4_outside_the_staging_limit_is_refused_untouched(ops, oracle, M, K):
    c = _case(ops, oracle, 8, K, 64, rows=M, oracle_rows=(0, M - 1), negate=2)
    y = torch.full((M, 64), 7.0, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match=STAGING):
        _gemv_into(c.x, c, y)
    with pytest.raises(RuntimeError, match=STAGING):
        ops.w8_a16_gemm(c.x, c.packed, c.s, path="gemv")
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert _auto(8, M, 64, K)[0] == STREAM
    c.check(ops.w8_a16_gemm(c.x, c.packed, c.s), M, "auto")


# ---------------------------------------------------------------------------------------------- int8, small and medium batches

STREAM_M = (2, 8, 16, 17, 33, 64)
# eetq_diag_stream_plan at 256 CUs, the same at all three depths: (form, tile rows per workgroup, waves)
STREAM_PLANS = {64: {2: (RING, 1, 16), 8: (RING, 1, 16), 16: (RING, 1, 8)},       # 4 tile rows: per-wave ring, 16-row ring from M = 9
                8192: {2: (REGS, 2, 8), 8: (REGS, 2, 8), 16: (RING, 2, 8)}}       # 2 tile rows per CU: registers, two rows per workgroup


# (17 <= M <= 32: the 32-row ring of the explicit path; 33 <= M <= 64: its one deep-K register form, 16 waves x 2 tiles)
@pytest.mark.parametrize("M", STREAM_M)
@pytest.mark.parametrize("K,N", [(K, N) for K in (28672, 53248, 65600) for N in (64, 8192)])
def test_stream_kernel_above_k_16384(ops, oracle, K, N, M):
    c = _case(ops, oracle, 8, K, N, rows=max(STREAM_M), oracle_rows=(0,) + tuple(m - 1 for m in STREAM_M))
    if M <= 16:
        assert _stream_plan(8, M, N, K) == STREAM_PLANS[N][M]
    x = c.x[:M]
    y = ops.w8_a16_gemm(x, c.packed, c.s, path="stream")
    c.check(y, M, "stream")
    _epilogue(ops, c, M, y, path="stream")
    # AUTO: the stream kernel up to M = 16 except the narrow deep weight from M = 9, the split-K tile above
    want = STREAM if M <= 8 or (M <= 16 and N == 8192) else SPLITK
    assert _auto(8, M, N, K)[0] == want
    auto = ops.w8_a16_gemm(x, c.packed, c.s)
    if want == STREAM:
        assert torch.equal(auto, y)
    else:
        c.check(auto, M, "auto")
        assert torch.equal(auto, ops.w8_a16_gemm(x, c.packed, c.s))


MID_M = (33, 64, 128, 200, 1024)


# N = 272: five 64-column tiles per row tile, 17 tile rows.  K / 64 = 448 and 832: four K slices are 112 and 208 steps each.
@pytest.mark.parametrize("M", MID_M)
@pytest.mark.parametrize("K", [28672, 53248])
def test_tile_kernels_above_k_16384(ops, oracle, K, M):
    N = 272
    rows = tuple(sorted({0, *(m // 2 for m in MID_M), *(m - 1 for m in MID_M)}))
    c = _case(ops, oracle, 8, K, N, rows=max(MID_M), oracle_rows=rows)
    # AUTO: two 32-row groups of the split-K tile up to M = 64; four K slices of the tiled kernel's 128 x 64 tile above
    assert _auto(8, M, N, K) == ((SPLITK, 2) if M <= 64 else (TILESPLIT, 4))
    x = c.x[:M]
    whole = ops.w8_a16_gemm(x, c.packed, c.s, path="mfma")
    c.check(whole, M, "mfma")
    _epilogue(ops, c, M, whole, path="mfma")
    auto = ops.w8_a16_gemm(x, c.packed, c.s)
    c.check(auto, M, "auto")
    assert torch.equal(auto, ops.w8_a16_gemm(x, c.packed, c.s))
    _epilogue(ops, c, M, auto)
    if M > 128:
        return
    c.check(ops.w8_a16_gemm(x, c.packed, c.s, path="mid"), M, "mid")
    for path in ("splitk", "tilesplit"):      # tilesplit: 5 tiles x 4 <= 256 CUs and K / 64 / 4 >= 24 -> four slices
        y = ops.w8_a16_gemm(x, c.packed, c.s, path=path)
        c.check(y, M, path)
        assert torch.equal(y, ops.w8_a16_gemm(x, c.packed, c.s, path=path))
        _epilogue(ops, c, M, y, path=path)
    if M in (64, 128):
        for plan in ("1,4,22", "2,2,22", "2,4,22,2"):     # (column blocks, K slices, ring[, row groups]), as test_splitk_every_plan
            os.environ["EETQ_AMD_SPLITK_PLAN"] = plan
            try:
                y1 = ops.w8_a16_gemm(x, c.packed, c.s, path="splitk")
                y2 = ops.w8_a16_gemm(x, c.packed, c.s, path="splitk")
                torch.cuda.synchronize()
            finally:
                os.environ.pop("EETQ_AMD_SPLITK_PLAN", None)
            assert torch.equal(y1, y2), plan
            c.check(y1, M, "splitk " + plan)


# ---------------------------------------------------------------------------------------------- int4

I4_M = (1, 2, 4, 8, 16, 40, 128, 200)


# GEMV (explicit path; 128 k per tile): K = 28672 at M = 1 is 8-column units (K / 128 = 224 >= 40, even: gemv_half_kernel<8, 2,
# XV = 8, 4, 0, BITS = 4>), at M = 2 16 waves x 4 tiles with need = 7 (XV = 8); K = 53248 and 65536 at M = 1 16 waves x 4 tiles,
# need = 7 and 8 (XV = 8); everything with M * K > 65536 is refused.  AUTO at M = 1 is the stream kernel at these depths already.
@pytest.mark.parametrize("M", I4_M)
@pytest.mark.parametrize("K,N", [(K, N) for K in (28672, 53248, 65536, 65664) for N in (64, 272)])
def test_int4_above_k_16384(ops, oracle, K, N, M):
    c = _case(ops, oracle, 4, K, N, rows=max(I4_M), oracle_rows=(0,) + tuple(m - 1 for m in I4_M), negate=2 if N == 64 else 3)
    want = STREAM if M <= 16 else SPLITK if M <= 128 else MFMA
    assert _auto(4, M, N, K)[0] == want
    if M <= 16:
        assert _stream_plan(4, M, N, K) == ((RING, 1, 16) if M <= 8 else (RING, 1, 8))
    x = c.x[:M]
    auto = ops.w8_a16_gemm(x, c.packed, c.s)
    c.check(auto, M, "auto")
    _epilogue(ops, c, M, auto)
    paths = (("gemv",) if M <= 4 else ()) + (("stream",) if M <= 16 else ()) + (("splitk",) if M <= 128 else ()) + ("mfma",)
    for path in paths:
        if path == "gemv" and M * K > 65536:
            with pytest.raises(RuntimeError, match="W4A16 GEMV: M\\*K " + STAGING):
                ops.w8_a16_gemm(x, c.packed, c.s, path=path)
            continue
        y = ops.w8_a16_gemm(x, c.packed, c.s, path=path)
        c.check(y, M, path)
        if path == "splitk":
            assert torch.equal(y, ops.w8_a16_gemm(x, c.packed, c.s, path=path))
        if path == {STREAM: "stream", SPLITK: "splitk", MFMA: "mfma"}[want]:
            assert torch.equal(y, auto), path
        if path == "gemv":
            _epilogue(ops, c, M, y, path=path)
    if M in (40, 128):
        for plan in ("1,4,22", "2,2,22", "2,4,22,2"):
            os.environ["EETQ_AMD_SPLITK_PLAN"] = plan
            try:
                y1 = ops.w8_a16_gemm(x, c.packed, c.s, path="splitk")
                y2 = ops.w8_a16_gemm(x, c.packed, c.s, path="splitk")
                torch.cuda.synchronize()
            finally:
                os.environ.pop("EETQ_AMD_SPLITK_PLAN", None)
            assert torch.equal(y1, y2), plan
            c.check(y1, M, "splitk " + plan)


# ---------------------------------------------------------------------------------------------- grouped GEMV

def _problems(ops, oracle, K, N, count, seed, oracle_every):
    """count independent M = 1 problems of one shape: slices of one random stack, each packed on its own"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    out = []
    for i in range(count):
        q = torch.randint(-128, 128, (K, N), dtype=torch.int8, device=DEV, generator=g)
        s = (torch.rand(N, device=DEV, generator=g) * 0.02 + 1e-3).half()
        x = torch.rand(1, K, device=DEV, generator=g).half()
        x[:, ::3] *= -1
        ref = None
        if i % oracle_every == 0:
            ref = oracle.w8a16_gemm(x.cpu().numpy(), q.cpu().numpy(), s.cpu().numpy()).astype(np.float32)
        out.append((x, ops.preprocess_weights(q), s, ref))
    return out


def _tier_a_np(y, ref):
    y, ref = np.asarray(y, np.float32), np.asarray(ref, np.float32)
    return np.abs(y - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)


# launch_gemv_grouped: at most 32 problems per dispatch; a dispatch with more than 2 * 256 tile rows runs 8-wave workgroups
# (need = ceil(K / 8 / 512)), a smaller one 16-wave ones (need = ceil(K / 8 / 1024)).  40 problems of N = 272 are a dispatch of
# 32 x 17 = 544 rows and one of 8 x 17 = 136.  (N = 256 would make the first 512 rows: not MORE than two per CU, 16 waves.)
@pytest.mark.parametrize("K,N,count,forms", [
    (28672, 64, 3, "12 rows: <16, 2, XV = 4>"),
    (28672, 272, 40, "<8, 2, XV = 8>, then <16, 2, XV = 4>"),
    (8192, 272, 40, "<8, 2, XV = 2>, then <16, 2, XV = 1>"),
    (16384, 272, 40, "<8, 2, XV = 4>, then <16, 2, XV = 2>"),
    (32768, 64, 3, "the deepest K the grouped kernel takes: <16, 2, XV = 4>"),
])
def test_grouped_gemv_forms(ops, oracle, K, N, count, forms):
    """Another summation order than a separate launch (which takes the 8-column units at these N): tier A against it and against
    the oracle; the same bits from call to call; bias and residual on some problems equal the separate fp16 adds."""
    probs = _problems(ops, oracle, K, N, count, seed=K + N + count, oracle_every=8 if count > 8 else 1)
    xs, ws, ss = [p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs]
    outs = ops.w8_a16_gemv_grouped(xs, ws, ss)
    assert len(outs) == count
    again = ops.w8_a16_gemv_grouped(xs, ws, ss)
    for i, (x, w, s, ref) in enumerate(probs):
        assert torch.equal(outs[i], again[i]), i
        single = ops.w8_a16_gemm(x, w, s)
        assert outs[i].shape == single.shape and _tier_a_np(outs[i].cpu().numpy(), single.cpu().numpy()).all(), (i, forms)
        if ref is not None:
            assert _tier_a_np(outs[i].cpu().numpy(), ref).all(), (i, forms)
    g = torch.Generator(device=DEV)
    g.manual_seed(count)
    biases = [torch.randn(N, device=DEV, generator=g).half() if i % 2 == 0 else None for i in range(count)]
    residuals = [torch.randn(1, N, device=DEV, generator=g).half() if i % 3 == 0 else None for i in range(count)]
    fused = ops.w8_a16_gemv_grouped(xs, ws, ss, biases, residuals)
    for i in range(count):
        want = outs[i]
        if biases[i] is not None:
            want = want + biases[i]
        if residuals[i] is not None:
            want = want + residuals[i]
        assert torch.equal(fused[i], want), (i, forms)


def test_grouped_gemv_past_its_k_limit_is_the_ordinary_launch(ops, oracle):
    """K = 32832 > 32768: the grouped call launches each problem through the ordinary dispatcher -- the separate call, bit for bit"""
    probs = _problems(ops, oracle, 32832, 64, 3, seed=5, oracle_every=1)
    outs = ops.w8_a16_gemv_grouped([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs])
    for i, (x, w, s, ref) in enumerate(probs):
        assert torch.equal(outs[i], ops.w8_a16_gemm(x, w, s)), i
        assert _tier_a_np(outs[i].cpu().numpy(), ref).all(), i


# ---------------------------------------------------------------------------------------------- input gradient: reduction over N

_grads = {}


def _grad_weight(ops, oracle, bits):
    """weight [K, N = 28672]: dx = dy . fp16(q s)^T reduces over N.  int8: K = 320 (K % 128 == 64: the tail); the int4 layout needs
    K % 128 == 0: K = 384."""
    if bits not in _grads:
        N, K = 28672, 320 if bits == 8 else 384
        rng = np.random.default_rng(N + bits)
        s = (rng.random(N, dtype=np.float32) * 0.02 + 1e-3).astype(np.float16)
        if bits == 8:
            q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
            packed = ops.preprocess_weights(torch.from_numpy(q).to(DEV))
        else:
            raw = rng.integers(-128, 128, size=(K, N // 2), dtype=np.int8)
            q = oracle.i4_values(raw)
            packed = ops.preprocess_weights(torch.from_numpy(raw).to(DEV), True)
        deq = oracle.dequant(q, s)
        _grads[bits] = (packed, torch.from_numpy(s).to(DEV), deq, torch.from_numpy(deq).to(DEV).float())
    return _grads[bits]


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("M", [1, 17, 128])
def test_input_gradient_over_a_deep_n(ops, oracle, bits, M):
    op = ops.w8_a16_gemm_t if bits == 8 else ops.w4_a16_gemm_t
    packed, s, _, deq32 = _grad_weight(ops, oracle, bits)
    g = torch.Generator(device=DEV)
    g.manual_seed(M)
    dy = torch.randn(M, 28672, device=DEV, generator=g).half()
    got = op(dy, packed, s)
    ref = dy.float() @ deq32.t()
    err = (got.float() - ref).abs()
    assert got.shape == ref.shape and bool((err <= 1e-3 * ref.abs().max() + 2e-3 * ref.abs()).all()), float(err.max())
    assert torch.equal(got, op(dy, packed, s))


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3])
def test_input_gradient_one_hot_rows_over_a_deep_n(ops, oracle, bits, scale):
    """512 one-hot rows -- the first 64 columns of N, the last 64 and 384 random ones: the dequantised weight rows, bit for bit"""
    op = ops.w8_a16_gemm_t if bits == 8 else ops.w4_a16_gemm_t
    packed, s, deq, _ = _grad_weight(ops, oracle, bits)
    N = 28672
    cols = np.concatenate([np.arange(64), np.arange(N - 64, N), np.random.default_rng(bits).integers(64, N - 64, 384)])
    dy = torch.zeros(512, N, dtype=torch.float16, device=DEV)
    dy[torch.arange(512, device=DEV), torch.from_numpy(cols).to(DEV)] = scale
    got = op(dy, packed, s).cpu().numpy()
    want = (deq.T[cols].astype(np.float32) * np.float32(scale)).astype(np.float16)
    assert got.shape == want.shape and got.view(np.uint16).tobytes() == want.view(np.uint16).tobytes()


# ---------------------------------------------------------------------------------------------- quantisers

@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("K,N", [(28672, 64), (28672, 80), (65536, 64), (65536, 80)])
def test_quantisers_above_k_16384(ops, oracle, K, N, bits, dtype):
    """P = K / 128 = 224 and 512 row blocks: the column maxima are reduced from the blocks' maxima in strides of 32.  One column
    has its maximum in the last row block, one in block 33 (the second trip of that loop), one in the very last row."""
    rng = np.random.default_rng(K + N + bits)
    w = (rng.standard_normal((K, N)) * 0.02).astype(dtype)
    w[K - 100, 3] = 0.75                  # the last row block
    w[33 * 128 + 5, 7] = -0.5             # block 33
    w[K - 1, N - 1] = 1.0
    w[:, N // 2] = 0
    qt = torch.int8 if bits == 8 else torch.quint4x2
    if bits == 8:
        q, s = oracle.quantize(w)
        packed = oracle.gfx950_pack(q)
    else:
        q, s = oracle.quantize_i4(w)
        packed = oracle.gfx950_pack_i4(q)
    wd = torch.from_numpy(w).to(DEV)
    raw, processed, scales = ops.quant_weights(wd, qt, True)
    assert np.array_equal(raw.cpu().numpy(), q)
    assert scales.cpu().numpy().tobytes() == s.tobytes()
    assert np.array_equal(processed.cpu().numpy(), packed)
    only, scales2 = ops.quant_weights(wd, qt, False)
    assert np.array_equal(only.cpu().numpy(), packed)
    assert scales2.cpu().numpy().tobytes() == s.tobytes()


# ---------------------------------------------------------------------------------------------- mixture of experts

# Mixtral-8x22B's down projection depth: K = 16384 (256 int8 k tiles, 128 int4 ones).  T = 1 and 5: the grouped decode kernel;
# T = 64: the tiled prompt kernel where its own *_supported query takes the shape, the documented quiet refusal where it does not.
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("T", [1, 5, 64])
def test_moe_grouped_gemms_at_k_16384(oracle, bits, T):
    from eetq_amd import _lib
    from test_gpu_moe import _route, _routing, _stack
    from test_gpu_moe_int4 import _stack4
    lib = _lib.lib()
    E, k, K, N = 4, 2, 16384, 64
    if bits == 8:
        raw, proc, scales = _stack(E, K, N, seed=T)
        vals = raw.numpy()
    else:
        (raw, proc, scales), _ = _stack4(E, K, N, seed=T)
        vals = np.stack([oracle.i4_values(r) for r in raw.numpy()])
    x = (torch.rand(T, K, generator=torch.Generator().manual_seed(K + T)) - 0.5).half()
    idx = _routing(T, k, E, "uniform", seed=T)
    counts, offsets, sorted_slot, position, active = _route(lib, idx, E)
    S, used = T * k, int(offsets[-1])
    assert used == S
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tab = (p(offsets), p(sorted_slot), p(active))
    xd = x.to(DEV)
    POISON = -777.0
    dec = torch.full((S, N), POISON, dtype=torch.float16, device=DEV)
    f = lib.eetq_w8a16_moe_gemm if bits == 8 else lib.eetq_w4a16_moe_gemm
    assert f(p(xd), p(proc), p(scales), *tab, p(dec), T, k, E, N, K, 1, 0, st) == 0
    outs = [("decode", dec)]
    if T == 64:
        tiled = torch.full((S, N), POISON, dtype=torch.float16, device=DEV)
        if bits == 8:
            ok = lib.eetq_w8a16_moe_gemm_tiled_supported(T, k, E, N, K, 1)
            rc = lib.eetq_w8a16_moe_gemm_tiled(p(xd), p(proc), p(scales), *tab, p(tiled), T, k, E, N, K, 1, 0, st)
        else:
            ok = lib.eetq_w4a16_moe_gemm_tiled_supported(T, k, E, N, K, 1)
            rc = lib.eetq_w4a16_moe_gemm_tiled(p(xd), p(proc), p(scales), *tab, p(tiled), T, k, E, N, K, 1, 0, 0, st)
        torch.cuda.synchronize()
        if ok:
            assert rc == 0
            outs.append(("tiled", tiled))
        else:
            assert rc == _lib.ERR_UNSUPPORTED and bool((tiled == POISON).all())
    torch.cuda.synchronize()
    off, slots = offsets.cpu().numpy(), sorted_slot.cpu().numpy()
    s_np = scales.cpu().numpy()
    for e in range(E):
        rows = slice(off[e], off[e + 1])
        if off[e + 1] == off[e]:
            continue
        ref = oracle.w8a16_gemm(x.numpy()[slots[rows] // k], vals[e], s_np[e])
        assert np.abs(ref.astype(np.float32)).max() > 0.1
        for name, y in outs:
            assert _tier_a_np(y[rows].cpu().numpy(), ref).all(), (name, e)
