"""w4_a16_gemm_t -- the W4A16 projection's input gradient, dx = dy . fp16(q s)^T, straight from the gfx950 int4 tiles -- and what is
built on it: W4A16Linear.trainable, a LoRA adapter on a frozen W4A16Linear, eet_quantize(bits=4, trainable=True) on a tiny Llama.
Exactness on one-hot rows (every nibble of every tile through every lane position), tier A against a float32 product of the
oracle's dequantised weight, the bits of the int8 kernel on the same integers, strides, determinism, memory.

Shapes: N = 16 .. 272 gives 1, 1, 2, 3 and 5 steps of 64 columns (both parities of the two-stage pipeline, the prologue with and
without a second and third load; 16 and 272 leave three of a step's four column groups past N, 208 one); K = 384 is three column
tiles (an uneven split over the eight XCD runs), K = 1024 eight (an even one)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(K, N) for K in (128, 384) for N in (16, 64, 128, 192, 272)] + [(1024, 208)]
ROW_SHAPES = [(128, 16), (384, 272), (1024, 208)]


def _tier_a(y, ref):
    y = np.asarray(y, np.float32)
    ref = np.asarray(ref, np.float32)
    tol = 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)
    return np.abs(y - ref) <= tol


def _ops():
    from eetq_amd import ops
    return ops


_weights = {}


def _weight(oracle, K, N):
    """Random int4 weight (all 16 codes) and fp16 scales: (gfx950 int4 tiles on the GPU, scales on the GPU, oracle-dequantised
    fp16 [K, N] numpy, its float32 transpose [N, K], the same integers as gfx950 int8 tiles on the GPU).  Computed once."""
    if (K, N) not in _weights:
        rng = np.random.default_rng(K * 7 + N)
        q = rng.integers(-8, 8, (K, N), np.int8)
        s = (rng.random(N, dtype=np.float32) * 0.02 + 1e-3).astype(np.float16)
        w4 = torch.from_numpy(oracle.gfx950_pack_i4(oracle.i4_from_values(q))).to(DEV)
        w8 = torch.from_numpy(oracle.gfx950_pack(q)).to(DEV)
        deq = oracle.dequant(q, s)
        _weights[(K, N)] = (w4, torch.from_numpy(s).to(DEV), deq, np.ascontiguousarray(deq.astype(np.float32).T), w8)
    return _weights[(K, N)]


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3])
def test_one_hot_rows_are_the_dequantised_weight_bit_for_bit(oracle, K, N, scale):
    w, s, deq, _, _ = _weight(oracle, K, N)
    perm = np.random.default_rng(N).permutation(N)
    dy = torch.zeros(N, N, dtype=torch.float16, device=DEV)
    dy[torch.arange(N, device=DEV), torch.from_numpy(perm).to(DEV)] = scale
    got = _ops().w4_a16_gemm_t(dy, w, s).cpu().numpy()
    want = (deq.T[perm].astype(np.float32) * np.float32(scale)).astype(np.float16)
    assert got.shape == (N, K)
    assert got.view(np.uint16).tobytes() == want.view(np.uint16).tobytes()


@pytest.mark.parametrize("K,N", ROW_SHAPES)
@pytest.mark.parametrize("M", [1, 2, 17, 127, 128, 129, 300])
def test_random_rows_tier_a(oracle, K, N, M):
    w, s, _, deq_t, _ = _weight(oracle, K, N)
    torch.manual_seed(M)
    dy = torch.randn(M, N, dtype=torch.float16, device=DEV)
    got = _ops().w4_a16_gemm_t(dy, w, s).cpu().numpy()
    want = dy.cpu().numpy().astype(np.float32) @ deq_t
    ok = _tier_a(got, want)
    assert ok.all(), (int((~ok).sum()), float(np.abs(got.astype(np.float32) - want).max()))


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("M", [1, 129])
def test_same_bits_as_the_int8_kernel_on_the_same_integers(oracle, K, N, M):
    w4, s, _, _, w8 = _weight(oracle, K, N)
    torch.manual_seed(M + N)
    dy = torch.randn(M, N, dtype=torch.float16, device=DEV)
    assert torch.equal(_ops().w4_a16_gemm_t(dy, w4, s), _ops().w8_a16_gemm_t(dy, w8, s))


def test_3d_strided_and_repeated_calls(oracle):
    K, N = 384, 272
    op = _ops().w4_a16_gemm_t
    w, s, _, deq_t, _ = _weight(oracle, K, N)
    torch.manual_seed(3)
    dy = torch.randn(3, 37, N, dtype=torch.float16, device=DEV)
    got = op(dy, w, s)
    assert got.shape == (3, 37, K)
    want = dy.reshape(-1, N).cpu().numpy().astype(np.float32) @ deq_t
    assert _tier_a(got.reshape(-1, K).cpu().numpy(), want).all()
    assert torch.equal(op(dy, w, s), got)                                # two calls: identical bits
    wide = torch.randn(3, 37, 2 * N, dtype=torch.float16, device=DEV)
    view = wide[..., ::2]                                               # non-contiguous
    assert torch.equal(op(view, w, s), op(view.contiguous(), w, s))
    row = torch.randn(N, dtype=torch.float16, device=DEV)
    bcast = row.expand(5, N)                                            # stride 0
    assert bcast.stride(0) == 0
    assert torch.equal(op(bcast, w, s), op(bcast.contiguous(), w, s))


def test_both_bindings_agree(oracle):
    from eetq_amd import ops_ctypes
    w, s, _, _, _ = _weight(oracle, 384, 272)
    torch.manual_seed(9)
    dy = torch.randn(9, 272, dtype=torch.float16, device=DEV)
    assert torch.equal(ops_ctypes.w4_a16_gemm_t(dy, w, s), _ops().w4_a16_gemm_t(dy, w, s))


def test_rows_beyond_m_stay_untouched(oracle):
    import ctypes

    from eetq_amd import _lib
    K, N, M = 384, 272, 129
    w, s, _, _, _ = _weight(oracle, K, N)
    torch.manual_seed(6)
    dy = torch.randn(M, N, dtype=torch.float16, device=DEV)
    dx = torch.full((256, K), -7.5, dtype=torch.float16, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().eetq_w4a16_gemm_t(ptr(dy), ptr(w), ptr(s), ptr(dx), M, N, K, stream))
    torch.cuda.synchronize()
    assert torch.equal(dx[:M], _ops().w4_a16_gemm_t(dy, w, s))
    assert bool((dx[M:] == -7.5).all())


@pytest.mark.parametrize("binding", ["ops", "ops_ctypes"])
def test_argument_errors_before_gpu_work(binding):
    import importlib
    op = importlib.import_module("eetq_amd." + binding).w4_a16_gemm_t
    w = torch.zeros(128, 32, dtype=torch.int8, device=DEV)                # packed int4 [K, N / 2], N = 64
    s = torch.ones(64, dtype=torch.float16, device=DEV)
    g = torch.zeros(4, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        op(g.cpu(), w, s)
    with pytest.raises(RuntimeError, match="float16"):
        op(g.float(), w, s)
    with pytest.raises(RuntimeError, match="N=32"):
        op(g[:, :32], w, s)
    with pytest.raises(RuntimeError, match="scale must have N"):
        op(g, w, s[:48])
    w8 = torch.zeros(128, 64, dtype=torch.int8, device=DEV)               # an int8 [K, N] weight with N scales
    with pytest.raises(RuntimeError, match="packed int4"):
        op(g, w8, s)
    with pytest.raises(RuntimeError, match="128"):
        op(g, torch.zeros(192, 32, dtype=torch.int8, device=DEV), s)      # K = 192
    with pytest.raises(RuntimeError, match="16"):                         # N = 24
        op(torch.zeros(4, 24, dtype=torch.float16, device=DEV), torch.zeros(128, 12, dtype=torch.int8, device=DEV),
           torch.ones(24, dtype=torch.float16, device=DEV))


# ---- autograd ---------------------------------------------------------------------------------------------------------
_modules = {}


def _linear(K, N, bias=True):
    """W4A16Linear.from_torch on a seeded fp16 K -> N layer, quantised once per shape."""
    from eetq_amd.modules.qlinear import W4A16Linear
    if (K, N, bias) not in _modules:
        torch.manual_seed(K + N)
        lin = torch.nn.Linear(K, N, bias=bias, dtype=torch.float16).to(DEV)
        _modules[(K, N, bias)] = W4A16Linear.from_torch(lin)
    return _modules[(K, N, bias)]


def _linear_from(w, s):
    """A bias-free W4A16Linear holding the given int4 tiles and scales."""
    from eetq_amd.modules.qlinear import W4A16Linear
    mod = W4A16Linear(w.shape[0], 2 * w.shape[1], bias=False, dev=DEV)
    mod.qweight.copy_(w)
    mod.weight_scales.copy_(s)
    return mod


@pytest.fixture
def trainable_linear():
    mod = _linear(512, 256)
    mod.trainable = True
    yield mod
    mod.trainable = False


@pytest.mark.parametrize("shape", [(33,), (1, 40), (3, 17)])
def test_trainable_module_backward_is_the_fused_op(trainable_linear, shape):
    mod = trainable_linear
    torch.manual_seed(len(shape))
    x = torch.randn(*shape, 512, dtype=torch.float16, device=DEV, requires_grad=True)
    y = mod(x)
    assert y.requires_grad
    mod.trainable = False
    plain = mod(x)
    assert not plain.requires_grad                                       # untrainable: detached, as always
    assert torch.equal(y, plain)                                         # same forward bits
    g = torch.randn_like(y)
    y.backward(g)
    assert x.grad.shape == x.shape
    assert torch.equal(x.grad, _ops().w4_a16_gemm_t(g, mod.qweight, mod.weight_scales))


def test_trainable_module_sum_backward_and_residual(trainable_linear):
    mod = trainable_linear
    x = torch.randn(2, 5, 512, dtype=torch.float16, device=DEV, requires_grad=True)
    mod(x).sum().backward()                                              # a stride-0 gradient
    ones = torch.ones(2, 5, 256, dtype=torch.float16, device=DEV)
    assert x.grad.shape == x.shape
    assert torch.equal(x.grad, _ops().w4_a16_gemm_t(ones, mod.qweight, mod.weight_scales))
    res = torch.randn(2, 5, 256, dtype=torch.float16, device=DEV)
    assert not mod(x, residual=res).requires_grad                        # an extension argument: the detached path
    assert not mod(x.detach()).requires_grad


def test_trainable_module_backward_memory():
    """K = N = 4096, M = 16: the identity path would allocate eye(K) and the dequantised weight (64 MiB); the fused op needs
    the gradient tensors only."""
    torch.manual_seed(4)
    w = torch.randint(-128, 128, (4096, 2048), dtype=torch.int8, device=DEV)      # any bytes are int4 tiles
    mod = _linear_from(w, torch.rand(4096, device=DEV).half() * 0.02 + 1e-3)
    mod.trainable = True
    x = torch.randn(16, 4096, dtype=torch.float16, device=DEV, requires_grad=True)
    y = mod(x)
    g = torch.randn_like(y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y.backward(g)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < 4 * 2 ** 20, extra


def test_lora_on_a_frozen_w4a16_linear(oracle):
    """y = base(x) + scaling * (x A^T) B^T with trainable fp16 A, B on a frozen 512 -> 1024 W4A16Linear; the gradients of A, B
    and x against a float32 reference on the oracle's dequantised weight."""
    K, N, r, M, scaling = 512, 1024, 16, 64, 0.5
    w, s, deq, _, _ = _weight(oracle, K, N)
    base = _linear_from(w, s)
    base.trainable = True
    torch.manual_seed(5)
    A = (torch.randn(r, K, device=DEV) * 0.02).half().requires_grad_(True)
    B = (torch.randn(N, r, device=DEV) * 0.02).half().requires_grad_(True)
    x = torch.randn(M, K, dtype=torch.float16, device=DEV, requires_grad=True)
    G = torch.randn(M, N, device=DEV).half()
    y = base(x) + scaling * ((x @ A.t()) @ B.t())
    (y.float() * G.float()).sum().backward()

    x32, A32, B32, G32 = (t.detach().cpu().float() for t in (x, A, B, G))
    W32 = torch.from_numpy(deq.astype(np.float32))                     # [K, N]
    h = x32 @ A32.t()                                                  # [M, r]
    gB = scaling * G32.t() @ h                                         # [N, r]
    gh = scaling * G32 @ B32                                           # [M, r]
    gA = gh.t() @ x32                                                  # [r, K]
    gx = G32 @ W32.t() + gh @ A32                                      # [M, K]
    for got, want in ((A.grad, gA), (B.grad, gB), (x.grad, gx)):
        ok = _tier_a(got.cpu().numpy(), want.numpy())
        assert ok.all(), (int((~ok).sum()), got.shape)


def test_tiny_llama_bits4_trainable(monkeypatch):
    """eet_quantize(bits=4, trainable=True) on a two-layer Llama: the gradient with respect to the input embeddings as shipped
    (w4_a16_gemm_t) against the same model with the backward product taken the identity way -- same forward, two backward
    products that differ only in summation order: tier A, as test_transformers_fused_backward holds its pair to."""
    transformers = pytest.importorskip("transformers")
    from eetq_amd.modules import qlinear
    from eetq_amd.modules.qlinear import W4A16Linear
    from eetq_amd.utils.quantizer import eet_quantize

    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=4, vocab_size=1000, max_position_embeddings=256)
    torch.manual_seed(11)
    model = transformers.LlamaForCausalLM(cfg).half().eval().to(DEV)
    eet_quantize(model, bits=4, trainable=True)
    mods = [m for m in model.modules() if isinstance(m, W4A16Linear)]
    assert len(mods) == 14 and all(m.trainable for m in mods)
    torch.manual_seed(12)
    emb = torch.randn(1, 24, 256, dtype=torch.float16, device=DEV) * 0.1
    G = torch.randn(1, 24, 1000, device=DEV).half().float()

    def grad_and_logits():
        e = emb.clone().requires_grad_(True)
        logits = model(inputs_embeds=e).logits
        (logits.float() * G).sum().backward()
        return e.grad.detach().clone(), logits.detach().clone()

    g_fused, y_fused = grad_and_logits()
    calls = []

    def identity_product(grad, weight, scales):
        calls.append(grad.shape)
        eye = torch.eye(weight.shape[0], device=weight.device, dtype=torch.float16)
        return grad.matmul(qlinear.w8_a16_gemm(eye, weight, scales).transpose(0, 1))

    monkeypatch.setattr(qlinear, "w4_a16_gemm_t", identity_product)
    g_ident, y_ident = grad_and_logits()
    assert len(calls) == 14                                             # the module looks the operator up at call time
    assert torch.equal(y_fused, y_ident)                                # same forward
    got, want = g_fused.cpu().numpy(), g_ident.cpu().numpy()
    ok = _tier_a(got, want)
    bad = np.argwhere(~ok)
    worst = np.unravel_index(np.argmax(np.abs(got.astype(np.float32) - want.astype(np.float32))), got.shape)
    print("tier A misses: %d of %d; worst element %s: %r vs %r" % (len(bad), ok.size, worst, got[worst], want[worst]))
    assert ok.all(), (len(bad), worst, float(got[worst]), float(want[worst]))
