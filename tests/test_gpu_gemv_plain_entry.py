"""The plain K = 4096 decode GEMV (M = 1, no bias / residual / activation) has its own kernel entry whose argument list is the four
pointers (gemv_kernel.hpp: gemv_plain_kernel): K is a constant to its address arithmetic and N is gone.  None of that may change a
bit: the same call with an all-zero fp16 bias runs the run-time-epilogue instantiation behind the eighteen-dword argument list
(fp16(acc) + 0 == fp16(acc)), and must give the same bytes.
K = 4096 is the only K this form serves, so the shapes are small in N: one tile row, three, and the benchmark's 256.  On a
256-CU device the automatic dispatch hands fewer than 129 tile rows to the column-unit kernels, so next to the shapes above
every test also runs at N = 2064 (129 tile rows), the smallest N that reaches the plain entry there, or at N = 4096.
Reference numerics: weightOnlyBatchedGemv/kernel.h:294-468 (fp32 accumulation here: tier A against the oracle)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 4096
NS = (16, 48, 4096)
N_ENTRY = 2064  # 129 tile rows


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as _ops
    return _ops


def _tier_a(y, ref):
    y = y.astype(np.float32)
    ref = ref.astype(np.float32)
    return np.abs(y - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)


@pytest.fixture(scope="module")
def problems(ops, oracle):
    """N -> (x, processed weight, scales) on the device, raw int8 q and scales on the host, the oracle's product: made once"""
    out = {}
    for N in NS + (N_ENTRY,):
        rng = np.random.default_rng(4096 + N)
        w = (rng.standard_normal((K, N)) * 0.02).astype(np.float16)
        x = rng.random((1, K)).astype(np.float16)
        qw, s = ops.quant_weights(torch.from_numpy(w).to(DEV), torch.int8, False)
        q, sc = oracle.quantize(w)
        assert s.cpu().numpy().tobytes() == sc.tobytes()
        out[N] = dict(x=torch.from_numpy(x).to(DEV), qw=qw, s=s, q=q, sc=sc, ref=oracle.w8a16_gemm(x, q, sc))
    return out


@pytest.mark.parametrize("N", NS + (N_ENTRY,))
def test_plain_entry_equals_zero_bias_call(ops, problems, N):
    p = problems[N]
    plain = ops.w8_a16_gemm(p["x"], p["qw"], p["s"])
    zero_bias = ops.w8_a16_gemm(p["x"], p["qw"], p["s"], bias=torch.zeros(N, dtype=torch.float16, device=DEV))
    assert plain.shape == (1, N) and torch.equal(plain, zero_bias)


@pytest.mark.parametrize("N", NS + (N_ENTRY,))
def test_plain_entry_tier_a_vs_oracle(ops, problems, N):
    p = problems[N]
    got = ops.w8_a16_gemm(p["x"], p["qw"], p["s"]).cpu().numpy()
    assert _tier_a(got, p["ref"]).all()


@pytest.mark.parametrize("N", (48, N_ENTRY))
def test_one_hot_rows_give_the_dequantised_weight_row(ops, problems, N):
    """x = e_k: every column is exactly fp16(q[k, n] * s[n]).  k = a lane-group edge (15 | 16), a tile edge (63 | 64), a wave edge
    (1023 | 1024) and the four tiles d of the first wave's neighbourhood and the last wave (k = 0, 1024 in tiles 0, 16 of wave 0;
    1023, 2047, 3071, 4095 in tiles 15, 31, 47, 63 of wave 15): a wrong base for any of the four loads puts another row's value
    into the columns."""
    p = problems[N]
    for k in (0, 15, 16, 63, 64, 1023, 1024, 2047, 3071, 4095):
        x = torch.zeros(1, K, dtype=torch.float16, device=DEV)
        x[0, k] = 1.0
        got = ops.w8_a16_gemm(x, p["qw"], p["s"]).cpu().numpy()
        want = (p["q"][k].astype(np.float32) * p["sc"].astype(np.float32)).astype(np.float16)  # exact in fp32: one rounding
        assert got.tobytes() == want.reshape(1, N).tobytes(), k


@pytest.mark.parametrize("N", (48, N_ENTRY))
def test_three_captured_launches_replayed_twice(ops, problems, N):
    p = problems[N]
    xs = [p["x"], p["x"] * 0.5, p["x"].flip(1).contiguous()]
    eager = [ops.w8_a16_gemm(x, p["qw"], p["s"]) for x in xs]
    outs = [torch.zeros(1, N, dtype=torch.float16, device=DEV) for _ in xs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for x, o in zip(xs, outs):  # warm-up on the capture stream (library initialisation is not capturable)
            ops.w8_a16_gemm_(x, p["qw"], p["s"], o, 1, N, K)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for x, o in zip(xs, outs):
            ops.w8_a16_gemm_(x, p["qw"], p["s"], o, 1, N, K)
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)


@pytest.mark.parametrize("N", (16, N_ENTRY))
def test_guard_elements_around_y_stay_untouched(ops, problems, N):
    G = 64
    p = problems[N]
    guard = torch.tensor(0x7bcd, dtype=torch.int16).view(torch.float16).item()
    buf = torch.full((G + N + G,), guard, dtype=torch.float16, device=DEV)
    y = buf[G:G + N].view(1, N)
    ops.w8_a16_gemm_(p["x"], p["qw"], p["s"], y, 1, N, K)
    torch.cuda.synchronize()
    assert torch.equal(y, ops.w8_a16_gemm(p["x"], p["qw"], p["s"]))
    raw = buf.view(torch.int16).cpu().numpy()
    assert (raw[:G] == 0x7bcd).all() and (raw[G + N:] == 0x7bcd).all()
