"""Reduction depths above K = 16384 without a GPU: what AUTO picks past the GEMV's staging limit, the refusals that come before any
launch, and how much of the tier-A bar the reference itself uses up at K = 65536 (tests/test_gpu_deep_k.py holds the kernels to that
bar against the oracle)."""
import ctypes

import numpy as np
import pytest

GEMV, MFMA, STREAM, MID, SPLITK, TILESPLIT = 1, 2, 3, 4, 5, 6
ERR_UNSUPPORTED = -3
STAGING = b"too large for LDS staging"


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def _auto(lib, bits, M, N, K):
    p, d = ctypes.c_int(-9), ctypes.c_int(-9)
    assert lib.eetq_diag_auto_path(bits, M, N, K, ctypes.byref(p), ctypes.byref(d)) == 0
    return p.value, d.value


def test_auto_leaves_the_gemv_where_no_form_stages_the_row(lib):
    """M = 1: the GEMV stages the activation row in LDS, 65536 values at most (16 waves x 64 lanes x eight 16-byte loads); a deeper
    row runs on the small-batch kernel with one row.  (Without a device the rule is an MI355X's: 256 CUs.)"""
    for N in (64, 4096, 8208, 16384):
        for K in (16384, 28672, 32768, 32832, 53248, 65536):
            assert _auto(lib, 8, 1, N, K) == (GEMV, 0), (N, K)
        for K in (65600, 69632, 131072):
            assert _auto(lib, 8, 1, N, K) == (STREAM, 0), (N, K)
    # int4 tiles: AUTO already runs one row on the stream kernel from K = 8192, or from 72 Mi weights, so every K > 65536 does
    for N in (64, 272, 4112, 6144, 8208):
        for K in (65664, 131072):
            assert _auto(lib, 4, 1, N, K) == (STREAM, 0), (N, K)
    # the operator wrappers' constant is the library's limit
    from eetq_amd import ops_ctypes
    assert ops_ctypes.GEMV_MAX_STAGED == 65536


def _aligned(nbytes):
    buf = (ctypes.c_char * (nbytes + 64))()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)


def test_staging_refusals_come_before_any_launch(lib):
    """Explicit GEMV launches and the fused-prologue M = 1 entry points past the staging limit: EETQ_ERR_UNSUPPORTED with the library's
    message from host arithmetic alone -- nothing is launched, so this runs without a device (the pointers are never followed)."""
    keep, p = _aligned(4096)
    for M, K in ((1, 65600), (1, 131072), (2, 32832), (3, 21888), (4, 16448), (4, 20480)):
        assert lib.eetq_w8a16_gemm_ex(p, p, p, p, M, 64, K, GEMV, None) == ERR_UNSUPPORTED, (M, K)
        assert b"GEMV: M*K " + STAGING in lib.eetq_last_error(), (M, K)
    for M, K in ((1, 65664), (2, 32896), (4, 16512)):
        assert lib.eetq_w4a16_gemm_ex(p, p, p, None, None, p, M, 64, K, GEMV, None) == ERR_UNSUPPORTED, (M, K)
        assert b"W4A16 GEMV: M*K " + STAGING in lib.eetq_last_error(), (M, K)
    K = 65600
    assert lib.eetq_w8a16_gemv_rmsnorm(p, p, 1e-5, p, p, None, None, p, 64, K, None) == ERR_UNSUPPORTED
    assert STAGING in lib.eetq_last_error()
    assert lib.eetq_w8a16_gemv_silu_gated(p, p, p, None, None, p, 64, K, None) == ERR_UNSUPPORTED
    assert STAGING in lib.eetq_last_error()
    assert lib.eetq_w8a16_gemv_glu8(p, p, 1e-5, p, p, None, p, 64, K, None) == ERR_UNSUPPORTED
    assert STAGING in lib.eetq_last_error()
    del keep


def test_tier_a_leaves_a_margin_at_k_65536(oracle):
    """The bar of test_gpu_deep_k.py, |err| <= 1e-3 * max|y| + 2e-3 * |y|, is only meaningful if the reference itself sits well inside
    it.  K = 65536, M = 4, N = 32, the inputs of that file (every int8 code, scales in [1e-3, 2.1e-2), activations uniform in [0, 1)
    with every third column negated): the oracle against a float64 product of the same fp16-dequantised weight differs by the final
    rounding to fp16 alone, at most 2^-11 |y| -- below 0.245 of the bar whatever the data.

    Measured maximum of |oracle - f64| / bound: 0.106 (max|y| = 539)."""
    K, M, N = 65536, 4, 32
    rng = np.random.default_rng(K + M + N)
    q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
    s = (rng.random(N, dtype=np.float32) * 0.02 + 1e-3).astype(np.float16)
    x = rng.random((M, K)).astype(np.float16)
    x[:, ::3] *= -1
    y = oracle.w8a16_gemm(x, q, s).astype(np.float64)
    ref = x.astype(np.float64) @ oracle.dequant(q, s).astype(np.float64)
    assert np.isfinite(y).all() and np.abs(ref).max() < 6e4          # far from fp16 overflow
    ratio = np.abs(y - ref) / (1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref))
    print("max |oracle - f64| / tier-A bound = %.4f, max|y| = %.1f" % (ratio.max(), np.abs(ref).max()))
    assert ratio.max() < 0.25
