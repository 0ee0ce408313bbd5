"""Routed W8A16 mixture-of-experts layer: the device routing tables, the grouped GEMM over the int8 expert stack,
the whole layer on both paths (T <= 16: four launches, no host sync; T > 16: per-expert AUTO GEMMs), determinism and graph
replay with rewritten routing, and tiny Mixtral / Qwen3-MoE models after eet_quantize(experts=True)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    L = _lib.lib()
    assert L.eetq_device_supported() == 1, "kernels are built for gfx950 only"
    return L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _route(lib, idx, E):
    T, k = idx.shape
    S, A = T * k, min(E, T * k)
    out = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)]
    assert lib.eetq_moe_route(_ptr(idx), T, k, E, *[_ptr(t) for t in out], _stream()) == 0
    return out


def _route_ref(idx, E):
    flat = idx.flatten().cpu()
    S = flat.numel()
    valid = (flat >= 0) & (flat < E)
    counts = torch.bincount(flat[valid], minlength=E).int()
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).int()
    key = torch.where(valid, flat, torch.full_like(flat, E))
    order = torch.sort(key, stable=True).indices
    nv = int(valid.sum())
    sorted_slot = torch.full((S,), -1, dtype=torch.int32)
    sorted_slot[:nv] = order[:nv].int()
    position = torch.full((S,), -1, dtype=torch.int32)
    position[order[:nv]] = torch.arange(nv, dtype=torch.int32)
    act = torch.nonzero(counts).flatten().int()
    active = torch.full((min(E, S),), -1, dtype=torch.int32)
    active[:act.numel()] = act
    return counts, offsets, sorted_slot, position, active


def _routing(T, k, E, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)])
    elif kind == "one":  # every token's first choice is expert E - 1
        idx = torch.stack([torch.cat([torch.tensor([E - 1]), torch.randperm(E - 1, generator=g)[:k - 1]]) for _ in range(T)])
    elif kind == "few":  # k + 1 experts (3 .. k + 3) only: the others get no rows
        idx = torch.stack([torch.randperm(k + 1, generator=g)[:k] + 3 for _ in range(T)])
    elif kind == "dup":  # every token's first two slots both pick expert E - 1: 2T rows on one expert
        idx = torch.randint(0, E, (T, k), generator=g)
        idx[:, :2] = E - 1
    elif kind == "sentinel":  # transformers' expert_idx == num_experts and -1 mixed in
        idx = torch.randint(0, E, (T, k), generator=g)
        idx[::2, 0] = E
        idx[1::3, -1] = -1
    else:  # any ids, duplicates within a token included
        idx = torch.randint(0, E, (T, k), generator=g)
    return idx.to(DEV)


@pytest.mark.parametrize("E", [8, 128, 1024])
@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("T", [1, 3, 16, 100, 3000])
@pytest.mark.parametrize("kind", ["uniform", "sentinel", "random"])
def test_route_tables_equal_stable_argsort(lib, E, k, T, kind):
    idx = _routing(T, k, E, kind, seed=E * 1000 + k * 100 + T)
    got = _route(lib, idx, E)
    torch.cuda.synchronize()
    for name, g, r in zip(("counts", "offsets", "sorted_slot", "position", "active"), got, _route_ref(idx, E)):
        assert torch.equal(g.cpu(), r), name


def _stack(E, K, N, seed):
    """fp16 expert weights [E, K, N] -> (raw int8 [E, K, N], processed gfx950 [E, K, N], scales [E, N]) on the GPU"""
    from eetq_amd.ops import quant_weights
    torch.manual_seed(seed)
    w = (torch.randn(E, K, N) * 0.05).half()
    raw, processed, scales = quant_weights(w, torch.int8, True)
    return raw, processed.to(DEV), scales.to(DEV)


def _glu8(processed, scales, K):
    from eetq_amd.utils.fuse import _glu8_interleave_columns, _glu8_interleave_tiles
    E, _, N = processed.shape
    h = processed.reshape(E, 2, -1)
    return (_glu8_interleave_tiles(h[:, 0], h[:, 1], K).reshape(E, K, N),
            _glu8_interleave_columns(scales[:, :N // 2], scales[:, N // 2:]).contiguous())


def _tier_a(y, ref):
    y, ref = np.asarray(y, np.float32), np.asarray(ref, np.float32)
    return np.abs(y - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)


def _silu_mul_np(g, u):
    g32 = g.astype(np.float32)
    return ((g32 / (1.0 + np.exp(-g32))).astype(np.float16) * u).astype(np.float16)


@pytest.mark.parametrize("K", [768, 2048, 4096])
@pytest.mark.parametrize("T,k,E,kind", [(16, 2, 8, "one"), (7, 2, 8, "random"), (4, 8, 128, "uniform"), (16, 1, 8, "few"),
                                         (16, 2, 8, "dup"), (16, 8, 128, "dup")])
def test_grouped_gemm_rows_against_oracle_and_auto(lib, K, T, k, E, kind):
    import oracle
    from eetq_amd.ops import w8_a16_gemm
    N = 256
    raw, processed, scales = _stack(E, K, N, seed=K + T)
    gproc, gscales = _glu8(processed, scales, K)
    x = (torch.rand(T, K) - 0.5).half()
    idx = _routing(T, k, E, kind, seed=K)
    counts, offsets, sorted_slot, position, active = _route(lib, idx, E)
    S = T * k
    xd = x.to(DEV)
    plain = torch.empty(S, N, dtype=torch.float16, device=DEV)
    glu = torch.empty(S, N // 2, dtype=torch.float16, device=DEV)
    args = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
    assert lib.eetq_w8a16_moe_gemm(_ptr(xd), _ptr(processed), _ptr(scales), *args, _ptr(plain), T, k, E, N, K, 1, 0, _stream()) == 0
    assert lib.eetq_w8a16_moe_gemm(_ptr(xd), _ptr(gproc), _ptr(gscales), *args, _ptr(glu), T, k, E, N, K, 1, 1, _stream()) == 0
    # the contiguous form reads the gathered rows in sorted order
    sorted_h = torch.cat([x[sorted_slot[:int(offsets[-1])].long().cpu() // k],
                          torch.zeros(S - int(offsets[-1]), K, dtype=torch.float16)]).to(DEV)
    contig = torch.empty(S, N, dtype=torch.float16, device=DEV)
    assert lib.eetq_w8a16_moe_gemm(_ptr(sorted_h), _ptr(processed), _ptr(scales), *args, _ptr(contig), T, k, E, N, K, 0, 0,
                                   _stream()) == 0
    # glu8 epilogue == the plain projection of the glu8-ordered stack followed by eetq_silu_mul_glu8_f16, bit for bit
    gplain = torch.zeros(S, N, dtype=torch.float16, device=DEV)
    assert lib.eetq_w8a16_moe_gemm(_ptr(xd), _ptr(gproc), _ptr(gscales), *args, _ptr(gplain), T, k, E, N, K, 1, 0, _stream()) == 0
    gsep = torch.empty(S, N // 2, dtype=torch.float16, device=DEV)
    assert lib.eetq_silu_mul_glu8_f16(_ptr(gplain), _ptr(gsep), S, N // 2, _stream()) == 0
    torch.cuda.synchronize()
    off = offsets.cpu().numpy()
    slots = sorted_slot.cpu().numpy()
    s_np, raw_np = scales.cpu().numpy(), raw.numpy()
    seen = 0
    for e in range(E):
        c = off[e + 1] - off[e]
        if not c:
            continue
        seen += c
        rows = slice(off[e], off[e + 1])
        xe = x.numpy()[slots[rows] // k]
        ref = oracle.w8a16_gemm(xe, raw_np[e], s_np[e])
        assert _tier_a(plain[rows].cpu().numpy(), ref).all(), e
        assert torch.equal(contig[rows], plain[rows]), e
        ref_glu = _silu_mul_np(ref[:, :N // 2], ref[:, N // 2:])
        assert _tier_a(glu[rows].cpu().numpy(), ref_glu).all(), e
        assert torch.equal(glu[rows], gsep[rows]), e
        auto = w8_a16_gemm(torch.from_numpy(xe).to(DEV), processed[e], scales[e])
        assert _tier_a(plain[rows].cpu().numpy(), auto.cpu().numpy()).all(), e
        auto_glu = w8_a16_gemm(torch.from_numpy(xe).to(DEV), gproc[e], gscales[e], activation="silu_glu8")
        assert _tier_a(glu[rows].cpu().numpy(), auto_glu.cpu().numpy()).all(), e
    assert seen == int((idx >= 0).logical_and(idx < E).sum())
    if kind == "dup":
        assert int(counts.max()) > 16  # the kernel's loop over 16-row tiles of one expert


def _experts(E, H, I, k, seed):
    """a transformers MixtralExperts with random fp16 weights on the GPU, its W8A16Experts, and the dequantised stacks"""
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd.modules.qlinear import W8A16Experts
    from eetq_amd.ops import quant_weights
    torch.manual_seed(seed)
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)
    src = MixtralExperts(cfg).half().to(DEV)
    with torch.no_grad():  # pre-activations and outputs of order 1 for x ~ N(0, 1)
        src.gate_up_proj.normal_(0, 1.5 / H ** 0.5)
        src.down_proj.normal_(0, 2.0 / I ** 0.5)
    q = W8A16Experts.from_experts(src)
    deq = []
    for p in (src.gate_up_proj, src.down_proj):
        raw, _, s = quant_weights(p.detach().transpose(1, 2).contiguous(), torch.int8, True)
        deq.append((raw.float() * s.float()[:, None, :]).half())  # fp16(q s), [E, K, N]
    return src, q, deq


def _layer_ref(x, idx, wts, deq, E):
    """float32 layer on the dequantised weights"""
    gu, dn = (d.float() for d in deq)
    I = dn.shape[1]
    T, k = idx.shape
    out = torch.zeros(x.shape, dtype=torch.float32, device=DEV)
    ids = idx.flatten()
    keep = ((ids >= 0) & (ids < E)).nonzero().flatten()  # slots t * k + j that take part
    e, tok = ids[keep], keep // k
    h = torch.bmm(x.float()[tok].unsqueeze(1), gu[e]).squeeze(1)
    a = torch.nn.functional.silu(h[:, :I]) * h[:, I:]
    d = torch.bmm(a.unsqueeze(1), dn[e]).squeeze(1) * wts.flatten().float()[keep, None]
    for j in range(k):  # slot order within each token, as the combine adds
        sel = keep % k == j
        out.index_add_(0, tok[sel], d[sel])
    return out


def _close(y, ref):
    """|y - ref| <= 1e-2 max|ref| + 1e-2 |ref| elementwise (ref: float32 on the dequantised weights; outputs are of order 1)"""
    y, ref = y.float(), ref.float()
    return bool(((y - ref).abs() <= 1e-2 * ref.abs().max() + 1e-2 * ref.abs()).all())


def _router_weights(T, k, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, k, generator=g) * 2).softmax(-1).to(DEV)


@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 64, 8)])
@pytest.mark.parametrize("T", [1, 2, 3, 7, 16, 17, 100])
@pytest.mark.parametrize("kind", ["uniform", "one", "few", "sentinel", "dup"])
def test_layer_against_fp32_reference(lib, E, H, I, k, T, kind):
    _, q, deq = _experts(E, H, I, k, seed=E + H)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, kind, seed=T)
    wts = _router_weights(T, k, seed=T + 1)
    y = q(x, idx, wts)
    assert y.shape == (T, H) and y.dtype == torch.float16
    ref = _layer_ref(x, idx, wts, deq, E)
    assert ref.abs().max() > 0.5
    assert _close(y, ref), (y.float() - ref).abs().max().item()
    # fp16 router weights take the same path (the reference on the same fp16 weights)
    assert _close(q(x, idx, wts.half()), _layer_ref(x, idx, wts.half().float(), deq, E))
    # the bound has teeth: all zeros, the unweighted mean over the k slots, reversed router weights and a dropped heaviest slot fail it
    # (not on "dup" routing, where slots of one token share an expert and weightings can coincide)
    assert not _close(torch.zeros_like(ref), ref)
    if kind != "dup":
        assert not _close(_layer_ref(x, idx, torch.full_like(wts, 1.0 / k), deq, E), ref)
        assert not _close(_layer_ref(x, idx, wts.flip(-1), deq, E), ref)
        dropped = idx.clone()  # each token's heaviest slot among those that take part
        live = wts.float().masked_fill((idx < 0) | (idx >= E), -1.0)
        dropped.scatter_(1, live.argmax(-1, keepdim=True), -1)
        assert not _close(_layer_ref(x, dropped, wts, deq, E), ref)


def test_layer_matches_transformers_eager():
    src, q, deq = _experts(8, 256, 128, 2, seed=5)
    with torch.no_grad():
        src.gate_up_proj.copy_(deq[0].transpose(1, 2))
        src.down_proj.copy_(deq[1].transpose(1, 2))
    for T in (1, 5, 40):
        x = torch.randn(T, 256, device=DEV).half()
        idx = _routing(T, 2, 8, "uniform", seed=T)
        wts = _router_weights(T, 2, seed=T)
        with torch.no_grad():
            ref = src(x, idx, wts)
        assert ref.abs().max() > 0.5
        assert _close(q(x, idx, wts), ref)


def test_repeat_calls_and_graph_replay_with_rewritten_routing(lib):
    _, q, _ = _experts(8, 256, 128, 2, seed=9)
    T, k, E = 4, 2, 8
    x = (torch.rand(T, 256, device=DEV) - 0.5).half()
    idx = _routing(T, k, E, "uniform", seed=1)
    wts = torch.rand(T, k, device=DEV).softmax(-1)
    a, b = q(x, idx, wts), q(x, idx, wts)
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        q(x, idx, wts)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = q(x, idx, wts)
    for seed, kind in ((2, "uniform"), (3, "sentinel"), (4, "random")):
        idx.copy_(_routing(T, k, E, kind, seed=seed))
        wts.copy_(torch.rand(T, k, device=DEV).softmax(-1))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, q(x, idx, wts)), kind


def _tiny(which):
    from transformers import MixtralConfig, MixtralForCausalLM, Qwen3MoeConfig, Qwen3MoeForCausalLM
    torch.manual_seed(0)
    if which == "mixtral":
        cfg = MixtralConfig(hidden_size=128, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=2, num_local_experts=8, num_experts_per_tok=2, vocab_size=512,
                            initializer_range=0.1)
        return MixtralForCausalLM(cfg).half().to(DEV).eval()
    cfg = Qwen3MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=64, num_hidden_layers=2,
                         num_attention_heads=4, num_key_value_heads=2, num_experts=16, num_experts_per_tok=4, vocab_size=512,
                         decoder_sparse_step=1, mlp_only_layers=[], initializer_range=0.1)
    return Qwen3MoeForCausalLM(cfg).half().to(DEV).eval()


@pytest.mark.parametrize("which", ["mixtral", "qwen3_moe"])
def test_tiny_models_after_eet_quantize_experts(which):
    import copy

    from eetq_amd.modules.qlinear import W8A16Experts
    from eetq_amd.ops import quant_weights
    from eetq_amd.utils.quantizer import eet_quantize
    model = _tiny(which)
    ref = copy.deepcopy(model)
    fp16_bytes = sum(p.numel() * 2 for n, p in model.named_parameters() if ".experts." in n)
    eet_quantize(model, experts=True)
    eet_quantize(ref)  # same attention projections; experts stay fp16 -- set to the dequantised int8 weights below
    with torch.no_grad():
        for layer in ref.model.layers:
            ex = layer.mlp.experts
            for p in (ex.gate_up_proj, ex.down_proj):
                raw, _, s = quant_weights(p.transpose(1, 2).contiguous(), torch.int8, True)
                p.copy_((raw.float() * s.float()[:, None, :]).half().transpose(1, 2))
    q_bytes = 0
    for layer in model.model.layers:
        assert isinstance(layer.mlp.experts, W8A16Experts)
        q_bytes += sum(b.numel() * b.element_size() for b in layer.mlp.experts.buffers())
    assert q_bytes <= 0.52 * fp16_bytes
    ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        got = model(ids).logits.float()
        want = ref(ids).logits.float()
    assert (got - want).abs().max() <= 2e-2 * want.abs().max()
    prompt = ids[:1, :10]
    out_q = model.generate(prompt, max_new_tokens=16, do_sample=False, min_new_tokens=16)
    out_r = ref.generate(prompt, max_new_tokens=16, do_sample=False, min_new_tokens=16)
    agree = (out_q[:, 10:] == out_r[:, 10:]).float().mean().item()
    assert agree >= 0.9, agree


def test_state_dict_round_trip_is_bit_identical():
    from eetq_amd.modules.qlinear import W8A16Experts
    src, q, _ = _experts(16, 128, 64, 4, seed=3)
    sd = {n: t.clone() for n, t in q.state_dict().items()}
    fresh = W8A16Experts.from_experts(src, init_only=True)
    fresh.load_state_dict(sd)
    for T in (3, 20):
        x = (torch.rand(T, 128, device=DEV) - 0.5).half()
        idx = _routing(T, 4, 16, "random", seed=T)
        wts = torch.rand(T, 4, device=DEV).softmax(-1)
        assert torch.equal(fresh(x, idx, wts), q(x, idx, wts))
