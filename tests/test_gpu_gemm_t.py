"""w8_a16_gemm_t -- the W8A16 projection's input gradient, dx = dy . fp16(q s)^T, from the int8 weight in its native layout --
and the autograd paths built on it: EetqLinear's backward, a LoRA adapter on a frozen EetqLinear, and transformers' EetqLinear
with the opt-in fused backward.  Exactness on one-hot rows (every weight byte, both tails), tier A against a float32 product of
the oracle's dequantised weight, strides, determinism, memory."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (K, N): both tails (K % 128 == 64, N % 64 == 16) and the 7B / 13B projections
SHAPES = [(320, 272), (4096, 4096), (4096, 11008), (11008, 4096), (13824, 5120)]
ROWS = [1, 2, 7, 16, 17, 64, 128, 129, 300, 1024, 2048]


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
    """Random int8 weight (every code -128 .. 127) and fp16 scales: (packed gfx950 on the GPU, scales on the GPU,
    oracle-dequantised fp16 [K, N] numpy, its float32 transpose [N, K])."""
    if (K, N) not in _weights:
        _weights.clear()   # one shape at a time: the 13B ones are 70 MB of int8 each
        rng = np.random.default_rng(K * 7 + N)
        q = rng.integers(-128, 128, size=(K, N), dtype=np.int8)
        s = (rng.random(N, dtype=np.float32) * 0.02 + 1e-3).astype(np.float16)
        packed = torch.from_numpy(oracle.gfx950_pack(q)).to(DEV)
        deq = oracle.dequant(q, s)
        _weights[(K, N)] = (packed, torch.from_numpy(s).to(DEV), deq, np.ascontiguousarray(deq.astype(np.float32).T))
    return _weights[(K, N)]


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3])
def test_one_hot_rows_are_the_dequantised_weight_bit_for_bit(oracle, K, N, scale):
    w, s, deq, _ = _weight(oracle, K, N)
    perm = np.random.default_rng(N).permutation(N)
    dy = torch.zeros(N, N, dtype=torch.float16, device=DEV)
    dy[torch.arange(N, device=DEV), torch.from_numpy(perm).to(DEV)] = scale
    got = _ops().w8_a16_gemm_t(dy, w, s).cpu().numpy()
    want = (deq.T[perm].astype(np.float32) * np.float32(scale)).astype(np.float16)
    assert got.shape == (N, K)
    assert got.view(np.uint16).tobytes() == want.view(np.uint16).tobytes()


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("M", ROWS)
def test_random_rows_tier_a(oracle, K, N, M):
    w, s, _, deq_t = _weight(oracle, K, N)
    torch.manual_seed(M)
    dy = torch.randn(M, N, dtype=torch.float16, device=DEV)
    got = _ops().w8_a16_gemm_t(dy, w, s).cpu().numpy()
    want = dy.cpu().numpy().astype(np.float32) @ deq_t
    ok = _tier_a(got, want)
    assert ok.all(), (int((~ok).sum()), float(np.abs(got.astype(np.float32) - want).max()))


@pytest.mark.parametrize("K,N", [(320, 272), (4096, 11008)])
def test_3d_strided_and_repeated_calls(oracle, K, N):
    op = _ops().w8_a16_gemm_t
    w, s, _, deq_t = _weight(oracle, K, N)
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
    w, s, _, _ = _weight(oracle, 320, 272)
    dy = torch.randn(9, 272, dtype=torch.float16, device=DEV)
    assert torch.equal(ops_ctypes.w8_a16_gemm_t(dy, w, s), _ops().w8_a16_gemm_t(dy, w, s))


@pytest.mark.parametrize("binding", ["ops", "ops_ctypes"])
def test_argument_errors_before_gpu_work(binding):
    import importlib
    op = importlib.import_module("eetq_amd." + binding).w8_a16_gemm_t
    w = torch.zeros(128, 64, dtype=torch.int8, device=DEV)
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
    w4 = torch.zeros(128, 32, dtype=torch.int8, device=DEV)               # packed int4: [K, N / 2] with N scales
    with pytest.raises(RuntimeError, match="int8 only"):
        op(g[:, :32], w4, s)


# ---- autograd ---------------------------------------------------------------------------------------------------------
def _eetq_linear(oracle, K, N, bias=True):
    from eetq_amd.modules.qlinear import EetqLinear
    w, s, deq, _ = _weight(oracle, K, N)
    mod = EetqLinear(K, N, bias=bias, device=DEV)
    mod.weight.copy_(w)
    mod.register_scale(DEV)
    mod.weight_scales.copy_(s)
    if bias:
        mod.bias.copy_(torch.randn(N, dtype=torch.float16))
    return mod.train(), deq


@pytest.mark.parametrize("shape", [(33,), (1, 40), (3, 17)])
def test_eetq_linear_backward_is_the_fused_op(oracle, shape):
    mod, _ = _eetq_linear(oracle, 320, 272)
    torch.manual_seed(len(shape))
    x = torch.randn(*shape, 320, dtype=torch.float16, device=DEV, requires_grad=True)
    y = mod(x)
    g = torch.randn_like(y)
    y.backward(g)
    assert x.grad.shape == x.shape
    assert torch.equal(x.grad, _ops().w8_a16_gemm_t(g, mod.weight, mod.weight_scales))


def test_eetq_linear_sum_backward(oracle):
    mod, _ = _eetq_linear(oracle, 4096, 4096, bias=False)
    x = torch.randn(2, 5, 4096, dtype=torch.float16, device=DEV, requires_grad=True)
    mod(x).sum().backward()
    ones = torch.ones(2, 5, 4096, dtype=torch.float16, device=DEV)
    assert x.grad.shape == x.shape
    assert torch.equal(x.grad, _ops().w8_a16_gemm_t(ones, mod.weight, mod.weight_scales))


def test_eetq_linear_backward_memory(oracle):
    """K = N = 4096, M = 16: the identity path would allocate eye(K) and the dequantised weight (64 MiB); the fused op needs
    the gradient tensors only."""
    mod, _ = _eetq_linear(oracle, 4096, 4096, bias=False)
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


def test_lora_on_a_frozen_eetq_linear(oracle):
    """y = base(x) + scaling * (x A^T) B^T with trainable fp16 A, B on a frozen 4096 -> 11008 EetqLinear; the gradients of A,
    B and x against a float32 reference on the oracle's dequantised weight."""
    K, N, r, M, scaling = 4096, 11008, 16, 64, 0.5
    base, deq = _eetq_linear(oracle, K, N, bias=False)
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


# ---- transformers' EetqLinear with the opt-in fused backward --------------------------------------------------------------
@pytest.fixture
def fused_backward_off():
    """Whatever a test switches on, transformers' own EetqLinearMMFunction is back afterwards."""
    from eetq_amd.utils.hf import set_fused_backward
    yield set_fused_backward
    set_fused_backward(False)


def test_transformers_fused_backward(tmp_path, fused_backward_off):
    transformers = pytest.importorskip("transformers")
    import transformers.integrations.eetq as hf_eetq
    from eetq_amd.utils.hf import FusedBackwardMMFunction, use_with_transformers

    shipped = hf_eetq.EetqLinearMMFunction
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=4, vocab_size=1000, max_position_embeddings=256)
    torch.manual_seed(11)
    transformers.LlamaForCausalLM(cfg).half().eval().save_pretrained(str(tmp_path))
    use_with_transformers()
    assert hf_eetq.EetqLinearMMFunction is shipped                     # the default stays transformers' code
    model = transformers.AutoModelForCausalLM.from_pretrained(str(tmp_path), quantization_config=transformers.EetqConfig("int8"),
                                                              device_map=DEV, dtype=torch.float16).eval()
    torch.manual_seed(12)
    emb = torch.randn(1, 24, 256, dtype=torch.float16, device=DEV) * 0.1
    G = torch.randn(1, 24, 1000, device=DEV).half().float()

    def grad_and_logits():
        e = emb.clone().requires_grad_(True)
        logits = model(inputs_embeds=e).logits
        (logits.float() * G).sum().backward()
        return e.grad.detach().clone(), logits.detach().clone()

    g_default, y_default = grad_and_logits()
    use_with_transformers(fused_backward=True)
    assert hf_eetq.EetqLinearMMFunction is FusedBackwardMMFunction
    g_fused, y_fused = grad_and_logits()
    assert torch.equal(y_fused, y_default)                             # same forward
    ok = _tier_a(g_fused.cpu().numpy(), g_default.cpu().numpy())
    assert ok.all(), int((~ok).sum())
    assert fused_backward_off(False) is True
    assert hf_eetq.EetqLinearMMFunction is shipped
