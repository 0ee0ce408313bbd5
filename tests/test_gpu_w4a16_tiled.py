"""The dense tiled MFMA kernel on int4 weights: ops.w4_a16_gemm_tiled / eetq_w4a16_gemm_tiled against the int8 tile
on the same integers -- w8_a16_gemm(x, p8, s, path="mfma") with p8 the int8 tile image of the nibbles -- BIT FOR BIT (torch.equal,
no tolerance) at both tile shapes and the launcher's own choice: both apply fp16(q s) with one rounding and add each output's
products in the same k order whatever the column blocking.  The forced int8 tiled path stays unsplit on every shape here (few
tiles, and fewer than 80 K steps wherever more than one round exists).  Two shapes are also held to the oracle (tier A, |err| <=
1e-3 max|ref| + 2e-3 |ref|) so that a defect shared with the int8 tile cannot pass.  Then exact dequantisation through an identity
input, two-hot rows, the bias / residual epilogue, the two-launch plan and its column seam, the rows around y, graph capture with
no scratch, W4A16Linear.prompt_path and a tiny Llama.

Shapes of the sweep: a ragged row tile (129, 200, 257, 300 rows), one column tile (N = 16: both lane halves of the weight DMA
clamped to it), N no multiple of 64 or 128 (80, 48, 1040), the six-step minimum (K = 384), one row (M = 1) and a deep K with a
128-deep last int4 tile (K = 11136 = 87 tiles)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.0

G1_SHAPES = [(129, 384, 1024), (200, 80, 384), (17, 16, 384), (128, 128, 512), (257, 1040, 1152), (1, 64, 384), (300, 48, 11136)]


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as _ops
    if _ops.BOUNDARY != "ext":
        pytest.skip("int4 goes through the compiled module (EETQ_AMD_BOUNDARY=ctypes selects the twin binding)")
    from eetq_amd import _lib
    assert _lib.lib().eetq_device_supported() == 1, "kernels are built for gfx950 only"
    return _ops


def _tier_a(y, ref):
    y, ref = np.asarray(y, np.float32), np.asarray(ref, np.float32)
    return np.abs(y - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)


_CASES = {}


def _case(M, N, K):
    """random nibbles and scales of a [K, N] weight, random activations, and the int8 tile's result: made once per shape, shared by
    the tests and never written"""
    import oracle

    import eetq_amd.ops as _ops
    key = (M, N, K)
    if key not in _CASES:
        rng = np.random.default_rng(M * 7 + N * 3 + K)
        vals = rng.integers(-8, 8, size=(K, N)).astype(np.int8)
        qp = oracle.i4_from_values(vals)
        assert np.array_equal(oracle.i4_values(qp), vals)
        p4 = torch.from_numpy(oracle.gfx950_pack_i4(qp)).to(DEV)
        p8 = torch.from_numpy(oracle.gfx950_pack(oracle.i4_values(qp))).to(DEV)
        s = (rng.uniform(0.005, 0.02, N)).astype(np.float16)
        x = (rng.uniform(-0.5, 0.5, (M, K))).astype(np.float16)
        c = dict(vals=vals, s=s, x=x, p4=p4, p8=p8, sd=torch.from_numpy(s).to(DEV), xd=torch.from_numpy(x).to(DEV))
        c["want"] = _ops.w8_a16_gemm(c["xd"], p8, c["sd"], path="mfma")
        torch.cuda.synchronize()
        _CASES[key] = c
    return _CASES[key]


def _report(got, want):
    return int((got != want).sum()), float((got.float() - want.float()).abs().max())


# ---- G1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", G1_SHAPES)
def test_bit_identical_to_the_int8_tile_at_every_tile_shape(ops, M, N, K):
    c = _case(M, N, K)
    assert ops.w4_a16_gemm_tiled_supported(M, N, K)
    want = c["want"]
    assert want.shape == (M, N) and not bool(want.isnan().any()) and float(want.float().abs().max()) > 0.05
    for tile in (0, 1, 2):
        got = ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"], tile=tile)
        assert got.shape == (M, N) and got.dtype == torch.float16
        assert torch.equal(got, want), (tile,) + _report(got, want)


# ---- G2 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(200, 80, 384), (257, 1040, 1152)])
def test_rows_against_the_oracle(ops, oracle, M, N, K):
    c = _case(M, N, K)
    rows = [0, M // 2, M - 1]
    ref = oracle.w8a16_gemm(c["x"][rows], c["vals"], c["s"])
    y = ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"])[rows].cpu().numpy()
    assert np.abs(ref.astype(np.float32)).max() > 0.05
    print("max |err|", float(np.abs(y.astype(np.float32) - ref.astype(np.float32)).max()))
    assert _tier_a(y, ref).all()
    assert not _tier_a(np.zeros_like(ref), ref).all()


# ---- G3 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(384, 64), (512, 48)])
def test_identity_input_returns_the_dequantised_weight_exactly(ops, oracle, K, N):
    """x = I_K: output row k is fp16(q[k] s), every nibble value at every k position of a tile (column 0 walks -8 .. 7 down its
    rows), both K halves and both parities of the K step"""
    rng = np.random.default_rng(K + N)
    vals = rng.integers(-8, 8, size=(K, N)).astype(np.int8)
    vals[:, 0] = (np.arange(K) % 16) - 8
    s = rng.uniform(0.005, 0.02, N).astype(np.float16)
    p4 = torch.from_numpy(oracle.gfx950_pack_i4(oracle.i4_from_values(vals))).to(DEV)
    want = oracle.dequant(vals, s)
    eye = torch.eye(K, dtype=torch.float16, device=DEV)
    for tile in (1, 2):
        got = ops.w4_a16_gemm_tiled(eye, p4, torch.from_numpy(s).to(DEV), tile=tile).cpu().numpy()
        assert np.array_equal(got, want), (tile, int((got != want).sum()))


# ---- G4 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(384, 80), (512, 80)])
def test_two_hot_rows_add_exactly_two_dequantised_weights(ops, oracle, K, N):
    """rows of x with two ones: the pair across the two K halves of a step (k, k + 32), across consecutive K steps (k, k + 64) and
    across the ring (k, K - 1 - k); the result is fp16(fp32(d1) + fp32(d2)) whichever wave and stage held each"""
    rng = np.random.default_rng(K * 5 + N)
    vals = rng.integers(-8, 8, size=(K, N)).astype(np.int8)
    s = rng.uniform(0.005, 0.02, N).astype(np.float16)
    p4 = torch.from_numpy(oracle.gfx950_pack_i4(oracle.i4_from_values(vals))).to(DEV)
    d = oracle.dequant(vals, s).astype(np.float32)
    pairs = []
    for k in (0, 7, 15, 16, 31, 40, 63, 64, 100, 129, K // 2 - 1, K - 65):
        pairs += [(k, k + 32), (k, k + 64), (k, K - 1 - k)]
    assert all(0 <= a < K and 0 <= b < K and a != b for a, b in pairs)
    x = np.zeros((len(pairs), K), np.float16)
    for r, (a, b) in enumerate(pairs):
        x[r, a] = x[r, b] = 1
    want = np.stack([(d[a] + d[b]).astype(np.float16) for a, b in pairs])
    for tile in (1, 2):
        got = ops.w4_a16_gemm_tiled(torch.from_numpy(x).to(DEV), p4, torch.from_numpy(s).to(DEV), tile=tile).cpu().numpy()
        assert np.array_equal(got, want), (tile, int((got != want).sum()))


# ---- G5 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(200, 80, 384), (129, 384, 1024)])
def test_bias_and_residual_equal_the_separate_fp16_adds(ops, M, N, K):
    c = _case(M, N, K)
    g = torch.Generator().manual_seed(M + N)
    bias = (torch.rand(N, generator=g) - 0.5).half().to(DEV)
    res = (torch.rand(M, N, generator=g) - 0.5).half().to(DEV)
    y = c["want"]
    for tile in (1, 2):
        both = ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"], bias=bias, residual=res, tile=tile)
        assert torch.equal(both, y + bias + res), (tile,) + _report(both, y + bias + res)
        assert torch.equal(ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"], bias=bias, tile=tile), y + bias), tile
        assert torch.equal(ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"], residual=res, tile=tile), y + res), tile


# ---- G6 -----------------------------------------------------------------------------------------------------------------------------
def test_two_launches_and_the_column_seam(ops, oracle):
    """(M, N, K) = (1024, 5120, 384) at tile = 0: on 256 CUs 320 wide tiles = one whole round over columns 0 .. 4095, then the last
    1024 columns in narrow tiles, which start at weight byte (4096 / 16) (K / 128) 1024.  The int8 launcher's ragged round would
    have 3 K steps per slice: unsplit."""
    M, N, K = 1024, 5120, 384
    c = _case(M, N, K)
    got = ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"], tile=0)
    assert torch.equal(got, c["want"]), _report(got, c["want"])
    rows, cols = [0, 511, 1023], slice(4032, 4160)
    ref = oracle.w8a16_gemm(c["x"][rows], c["vals"][:, cols], c["s"][cols])
    y = got[rows][:, cols].cpu().numpy()
    assert np.abs(ref.astype(np.float32)).max() > 0.05
    print("max |err|", float(np.abs(y.astype(np.float32) - ref.astype(np.float32)).max()))
    assert _tier_a(y, ref).all() and not _tier_a(np.zeros_like(ref), ref).all()
    g = torch.Generator().manual_seed(5)
    bias = (torch.rand(N, generator=g) - 0.5).half().to(DEV)
    res = (torch.rand(M, N, generator=g) - 0.5).half().to(DEV)
    both = ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"], bias=bias, residual=res, tile=0)
    assert torch.equal(both, got + bias + res), _report(both, got + bias + res)


# ---- G7 -----------------------------------------------------------------------------------------------------------------------------
def test_nothing_is_written_outside_y(ops):
    from eetq_amd import _lib
    M, N, K = 129, 80, 384
    c = _case(M, N, K)
    want = ops.w4_a16_gemm_tiled(c["xd"], c["p4"], c["sd"])
    f = _lib.lib().eetq_w4a16_gemm_tiled
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tile_j in (0, 1, 2):
        buf = torch.full((M + 2, N), SENTINEL, dtype=torch.float16, device=DEV)
        y = buf[1:M + 1]
        assert y.data_ptr() % 16 == 0
        st = f(ctypes.c_void_p(c["xd"].data_ptr()), ctypes.c_void_p(c["p4"].data_ptr()), ctypes.c_void_p(c["sd"].data_ptr()), None, None,
               ctypes.c_void_p(y.data_ptr()), M, N, K, tile_j, stream)
        assert st == 0, _lib.lib().eetq_last_error()
        torch.cuda.synchronize()
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[M + 1] == SENTINEL).all()), tile_j
        assert torch.equal(buf[1:M + 1], want), tile_j


# ---- G8 -----------------------------------------------------------------------------------------------------------------------------
def test_captures_into_a_graph_with_no_scratch(ops):
    M, N, K = 200, 384, 1024
    g = torch.Generator().manual_seed(3)
    c = _case(129, N, K)      # the weight of the (129, 384, 1024) case; fresh activations
    x = (torch.rand(M, K, generator=g) - 0.5).half().to(DEV)
    eager = ops.w4_a16_gemm_tiled(x, c["p4"], c["sd"])    # the large-LDS opt-in is done
    torch.cuda.synchronize()
    ops.release_workspace()                               # whatever earlier tests left: the capture starts with no scratch at all
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.w4_a16_gemm_tiled(x, c["p4"], c["sd"])
    for _ in range(2):
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    assert ops.release_workspace() == 0                   # the path owns no scratch
    del graph


# ---- G9 -----------------------------------------------------------------------------------------------------------------------------
def test_module_prompt_path_direct(ops, oracle):
    from eetq_amd.modules.qlinear import W4A16Linear
    torch.manual_seed(21)
    lin = torch.nn.Linear(1024, 384, bias=True, dtype=torch.float16).to(DEV)
    mod = W4A16Linear.from_torch(lin)
    auto = W4A16Linear.from_torch(lin)
    mod.prompt_path = "direct"
    assert auto.prompt_path == "auto" and torch.equal(mod.qweight, auto.qweight)
    x = (torch.rand(2, 100, 1024, generator=torch.Generator().manual_seed(1)) - 0.5).half().to(DEV)
    y = mod(x)
    assert y.shape == (2, 100, 384)
    assert torch.equal(y, ops.w4_a16_gemm_tiled(x, mod.qweight, mod.weight_scales, bias=mod.bias))
    vals = oracle.i4_values(oracle.gfx950_unpack_i4(mod.qweight.cpu().numpy()))
    ref = oracle.w8a16_gemm(x.reshape(200, 1024).cpu().numpy(), vals, mod.weight_scales.cpu().numpy()) + mod.bias.detach().cpu().numpy()
    assert _tier_a(y.reshape(200, 384).cpu().numpy(), ref).all() and not _tier_a(np.zeros_like(ref), ref).all()
    small = (torch.rand(8, 1024, generator=torch.Generator().manual_seed(2)) - 0.5).half().to(DEV)
    assert torch.equal(mod(small), auto(small))                      # 8 rows: today's call
    lin2 = torch.nn.Linear(256, 64, bias=False, dtype=torch.float16).to(DEV)
    a, b = W4A16Linear.from_torch(lin2), W4A16Linear.from_torch(lin2)
    b.prompt_path = "direct"
    x2 = (torch.rand(200, 256, generator=torch.Generator().manual_seed(3)) - 0.5).half().to(DEV)
    assert torch.equal(b(x2), a(x2))                                 # K = 256 < 384: outside the kernel, today's call, quietly
    # trainable: the same route in the forward, the unchanged backward
    mod.trainable = True
    xg = x.reshape(200, 1024).clone().requires_grad_(True)
    yg = mod(xg)
    assert yg.requires_grad and torch.equal(yg.detach(), y.reshape(200, 384))
    dy = (torch.rand(200, 384, generator=torch.Generator().manual_seed(4)) - 0.5).half().to(DEV)
    yg.backward(dy)
    assert torch.equal(xg.grad, ops.w4_a16_gemm_t(dy, mod.qweight, mod.weight_scales))
    mod.prompt_path = "expand"
    with pytest.raises(ValueError, match="prompt_path"):
        mod(x)


# ---- G10 ----------------------------------------------------------------------------------------------------------------------------
def test_tiny_llama_prompts_run_the_direct_tile(ops, monkeypatch):
    transformers = pytest.importorskip("transformers")
    from eetq_amd.modules import qlinear
    from eetq_amd.modules.qlinear import W4A16Linear
    from eetq_amd.utils import eet_quantize, set_prompt_path

    cfg = transformers.LlamaConfig(hidden_size=512, intermediate_size=1024, num_hidden_layers=1, num_attention_heads=4,
                                   num_key_value_heads=4, vocab_size=1000, max_position_embeddings=256)
    torch.manual_seed(13)
    model = transformers.LlamaForCausalLM(cfg).half().eval().to(DEV)
    eet_quantize(model, bits=4)
    mods = {n: m for n, m in model.named_modules() if isinstance(m, W4A16Linear)}
    assert len(mods) == 7
    ids = torch.randint(0, 1000, (1, 160), generator=torch.Generator().manual_seed(14)).to(DEV)
    outs = {}
    hooks = [m.register_forward_hook(lambda _m, _i, o, n=n: outs.__setitem__(n, o.detach().clone())) for n, m in mods.items()]
    calls = []
    real = qlinear.w4_a16_gemm_tiled

    def counted(*args, **kwargs):
        calls.append(args[0].shape)
        return real(*args, **kwargs)

    monkeypatch.setattr(qlinear, "w4_a16_gemm_tiled", counted)   # the module looks the operator up at call time
    with torch.no_grad():
        logits_auto = model(input_ids=ids).logits
        auto_outs = dict(outs)
        assert calls == []
        assert set_prompt_path(model, "direct") == 7
        outs.clear()
        logits = model(input_ids=ids).logits
        assert len(calls) == 7 and len(outs) == 7
        direct_outs = dict(outs)
        one = model(input_ids=ids[:, :1]).logits
        assert len(calls) == 7                                   # a 1-token forward never calls it
    for h in hooks:
        h.remove()
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(one).all()) and bool(torch.isfinite(logits_auto).all())
    for n in mods:
        got, want = direct_outs[n].float().cpu().numpy(), auto_outs[n].float().cpu().numpy()
        assert got.shape == want.shape and got.shape[-2] == 160
        assert np.abs(want).max() > 0
        assert _tier_a(got, want).all(), (n, float(np.abs(got - want).max()))
