"""Routed W4A16 mixture-of-experts layer: the quantisation of the int4 expert stacks against the oracle, the grouped
decode GEMM on int4 tiles per expert against the oracle (every routing kind, gather / contiguous, plain / glu8, untouched rows,
more rows than one MFMA tile, placement independence), the prompt path (expansion byte for byte, the layer bit for bit against the
C-ABI chain on the int8 stack with the same integers), the whole layer against a float64 reference with the layer's fp16 rounding
points, determinism, graph replay, and tiny Mixtral / Qwen3-MoE models after eet_quantize(experts=True, expert_bits=4).

Tolerance: the project's tier A, |err| <= 1e-3 max|ref| + 2e-3 |ref|, everywhere a tolerance is used.

The prompt-path cases are T = 64 and 512 on a Mixtral-like (E 8, k 2) and a Qwen3-like (E 128, k 8) shape.  The measured shape rule
(torch_ext.cpp) sends a layer to the expanded path from 64 rows per expert on average, which of the four only
(E 8, k 2, T 512) reaches -- at E 128, k 8, T = 64 is 4 rows per expert, below even the int8 layer's seam.  So that none of the
four is dropped and none can silently run the decode kernel, every case runs the expanded path by name (path="expand", which
raises where the tiled kernel cannot take the shape) and must equal the int8 chain bit for bit; what path="auto" does is then pinned
through ops.w4_a16_moe_path: it must equal the named path it reports, bit for bit, and report "expand" for (E 8, k 2, T 512)."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_moe import _route, _router_weights, _routing, _silu_mul_np, _tier_a

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = -777.0


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


def _glu8_cols(w):
    from eetq_amd.utils.fuse import _glu8_interleave_columns
    n = w.shape[-1] // 2
    return _glu8_interleave_columns(w[..., :n], w[..., n:]).contiguous()


def _stack4(E, K, N, seed):
    """fp16 expert weights [E, K, N] -> natural-order and glu8-order int4 stacks: (raw [E, K, N/2] CPU, gfx950 [E, K, N/2] GPU,
    scales [E, N] GPU) each"""
    from eetq_amd.ops import quant_weights
    torch.manual_seed(seed)
    w = (torch.randn(E, K, N) * 0.05).half()
    out = []
    for ww in (w, _glu8_cols(w)):
        raw, processed, scales = quant_weights(ww, torch.quint4x2, True)
        out.append((raw, processed.to(DEV), scales.to(DEV)))
    return out


def _mixtral_experts(E, H, I, k, seed):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts
    torch.manual_seed(seed)
    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)
    src = MixtralExperts(cfg).half().to(DEV)
    with torch.no_grad():  # pre-activations and outputs of order 1 for x ~ N(0, 1)
        src.gate_up_proj.normal_(0, 1.5 / H ** 0.5)
        src.down_proj.normal_(0, 2.0 / I ** 0.5)
    return src


def _experts4(E, H, I, k, seed):
    from eetq_amd.modules.qlinear import W4A16Experts
    src = _mixtral_experts(E, H, I, k, seed)
    return src, W4A16Experts.from_experts(src)


def _module_values(q):
    """the integers (-8 .. 7) and fp16 scales of a W4A16Experts, from its buffers through the oracle: gate|up [E, H, 2I] in glu8
    order, down [E, I, H]"""
    import oracle
    gu = np.stack([oracle.i4_values(oracle.gfx950_unpack_i4(t)) for t in q.gate_up_qweight.cpu().numpy()])
    dn = np.stack([oracle.i4_values(oracle.gfx950_unpack_i4(t)) for t in q.down_qweight.cpu().numpy()])
    return gu, q.gate_up_scales.cpu().numpy(), dn, q.down_scales.cpu().numpy()


def _layer_ref64(x, idx, wts, vals, E):
    """float64 layer on the oracle's dequantised int4 experts with the layer's fp16 rounding points: gate|up (glu8 order) -> fp16 ->
    silu_mul in fp16 -> down -> fp16 -> sum over the token's slots of fp32(row) * weight -> fp16"""
    import oracle
    gu_q, gu_s, dn_q, dn_s = vals
    x, idx, wts = x.cpu().numpy(), idx.cpu().numpy(), wts.float().cpu().numpy().astype(np.float64)
    T, k = idx.shape
    out = np.zeros((T, x.shape[1]), np.float64)
    for e in range(E):
        t, j = np.nonzero(idx == e)
        if not t.size:
            continue
        h = oracle.w8a16_gemm(x[t], gu_q[e], gu_s[e])                 # fp16, exact accumulation
        h = h.reshape(len(t), -1, 2, 8)
        a = _silu_mul_np(h[:, :, 0, :].reshape(len(t), -1), h[:, :, 1, :].reshape(len(t), -1))
        d = oracle.w8a16_gemm(np.ascontiguousarray(a), dn_q[e], dn_s[e]).astype(np.float64)
        np.add.at(out, t, d * wts[t, j, None])
    return out.astype(np.float16)


def test_from_experts_bytes_and_scales_equal_the_oracle():
    import oracle
    E, H, I = 4, 128, 256
    src, q = _experts4(E, H, I, 2, seed=1)
    assert q.gate_up_qweight.shape == (E, H, I) and q.down_qweight.shape == (E, I, H // 2)
    gu, dn = src.gate_up_proj.detach().cpu(), src.down_proj.detach().cpu()
    for e in range(E):
        wt = _glu8_cols(gu[e].t().contiguous()).numpy()                  # permuted w^T [H, 2I]
        qq, s = oracle.quantize_i4(wt)
        assert np.array_equal(q.gate_up_qweight[e].cpu().numpy(), oracle.gfx950_pack_i4(qq)), e
        assert q.gate_up_scales[e].cpu().numpy().tobytes() == s.tobytes(), e
        qq, s = oracle.quantize_i4(dn[e].t().contiguous().numpy())       # [I, H]
        assert np.array_equal(q.down_qweight[e].cpu().numpy(), oracle.gfx950_pack_i4(qq)), e
        assert q.down_scales[e].cpu().numpy().tobytes() == s.tobytes(), e
        assert oracle.i4_values(qq).min() == -8 and oracle.i4_values(qq).max() == 7


GEMM_CASES = [(16, 2, 8, "one"), (7, 2, 8, "random"), (4, 8, 128, "uniform"), (16, 1, 8, "few"), (16, 2, 8, "dup"),
              (16, 8, 128, "dup"), (16, 2, 8, "sentinel"), (5, 8, 128, "sentinel")]


def _check_grouped(lib, K, N, T, k, E, idx, x, seed):
    """run the four forms of eetq_w4a16_moe_gemm on one routing and check every written row per expert against the oracle"""
    import oracle
    (raw, proc, scales), (_, gproc, gscales) = _stack4(E, K, N, seed)
    counts, offsets, sorted_slot, position, active = _route(lib, idx, E)
    S = T * k
    used = int(offsets[-1])
    xd = x.to(DEV)
    tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
    f = lib.eetq_w4a16_moe_gemm

    def buf(n):
        return torch.full((S, n), POISON, dtype=torch.float16, device=DEV)
    plain, glu, contig, cglu, gplain = buf(N), buf(N // 2), buf(N), buf(N // 2), buf(N)
    assert f(_ptr(xd), _ptr(proc), _ptr(scales), *tab, _ptr(plain), T, k, E, N, K, 1, 0, _stream()) == 0
    assert f(_ptr(xd), _ptr(gproc), _ptr(gscales), *tab, _ptr(glu), T, k, E, N, K, 1, 1, _stream()) == 0
    # the contiguous forms read the gathered rows in sorted order (rows past offsets[E]: NaN, which nothing may read into a live row)
    sorted_h = torch.cat([x[sorted_slot[:used].long().cpu() // k],
                          torch.full((S - used, K), float("nan"), dtype=torch.float16)]).to(DEV)
    assert f(_ptr(sorted_h), _ptr(proc), _ptr(scales), *tab, _ptr(contig), T, k, E, N, K, 0, 0, _stream()) == 0
    assert f(_ptr(sorted_h), _ptr(gproc), _ptr(gscales), *tab, _ptr(cglu), T, k, E, N, K, 0, 1, _stream()) == 0
    # glu8 write-out == the plain projection of the glu8-ordered stack followed by eetq_silu_mul_glu8_f16, bit for bit
    assert f(_ptr(xd), _ptr(gproc), _ptr(gscales), *tab, _ptr(gplain), T, k, E, N, K, 1, 0, _stream()) == 0
    gsep = buf(N // 2)
    assert lib.eetq_silu_mul_glu8_f16(_ptr(gplain), _ptr(gsep), S, N // 2, _stream()) == 0
    torch.cuda.synchronize()
    off, slots = offsets.cpu().numpy(), sorted_slot.cpu().numpy()
    s_np, raw_np = scales.cpu().numpy(), raw.numpy()
    seen = 0
    for e in range(E):
        c = off[e + 1] - off[e]
        if not c:
            continue
        seen += c
        rows = slice(off[e], off[e + 1])
        xe = x.numpy()[slots[rows] // k]
        ref = oracle.w8a16_gemm(xe, oracle.i4_values(raw_np[e]), s_np[e])
        got = plain[rows].cpu().numpy()
        err = np.abs(got.astype(np.float32) - ref.astype(np.float32))
        assert _tier_a(got, ref).all(), (e, float(err.max()), float(np.abs(ref).max()))
        assert torch.equal(contig[rows], plain[rows]), e
        ref_glu = _silu_mul_np(ref[:, :N // 2], ref[:, N // 2:])
        assert _tier_a(glu[rows].cpu().numpy(), ref_glu).all(), e
        assert torch.equal(cglu[rows], glu[rows]), e
        assert torch.equal(glu[rows], gsep[rows]), e
    assert seen == used == int((idx >= 0).logical_and(idx < E).sum())
    for b in (plain, glu, contig, cglu, gplain):   # rows at or past offsets[E] keep the fill
        assert bool((b[used:] == POISON).all())
    assert not bool((plain[:used] == POISON).any())
    return counts, position, plain


# K = 768, 2048, 4096 (6, 16, 32 k tiles) run the four-wave single-stage instantiation; 8192 and 8320 (64 and 65 k tiles) the
# eight-wave one with two stages in flight that serves deep projections (Mixtral's down, K = 14336): at 64 tiles every wave owns 8
# (no tile left for the tail stage: its clamped load is redundant), at 65 wave 0 owns 9 and consumes the tail stage
@pytest.mark.parametrize("K", [768, 2048, 4096, 8192, 8320])
@pytest.mark.parametrize("T,k,E,kind", GEMM_CASES)
def test_grouped_decode_gemm_rows_against_oracle(lib, K, T, k, E, kind):
    x = (torch.rand(T, K, generator=torch.Generator().manual_seed(K + T)) - 0.5).half()
    idx = _routing(T, k, E, kind, seed=K)
    counts, _, _ = _check_grouped(lib, K, 256, T, k, E, idx, x, seed=K + T)
    if kind == "dup":
        assert int(counts.max()) > 16  # the kernel's loop over 16-row tiles of one expert
    if kind == "sentinel":
        assert int(counts.sum()) < T * k


@pytest.mark.parametrize("K", [768, 2048, 8192, 8320])
@pytest.mark.parametrize("rows", [40, 100])
def test_more_rows_than_one_tile_on_one_expert(lib, K, rows):
    T, k, E = rows, 1, 8
    x = (torch.rand(T, K, generator=torch.Generator().manual_seed(rows)) - 0.5).half()
    idx = torch.full((T, 1), 5, dtype=torch.long, device=DEV)
    counts, _, _ = _check_grouped(lib, K, 256, T, k, E, idx, x, seed=rows)
    assert counts.cpu().tolist() == [0, 0, 0, 0, 0, rows, 0, 0]


def test_row_bits_do_not_depend_on_t_routing_or_place(lib):
    """one (token row, expert) pair under four routings and three T: the same result bits wherever the row lands among its expert's
    rows (first tile, a later tile, a ragged last tile)"""
    K, N, E, k = 2048, 256, 8, 2
    (_, proc, scales), _ = _stack4(E, K, N, seed=3)
    g = torch.Generator().manual_seed(5)
    row = (torch.rand(K, generator=g) - 0.5).half()
    got, places = [], []
    for T, t, kind, seed in ((1, 0, "uniform", 1), (16, 7, "uniform", 1), (100, 93, "one", 2), (77, 76, "dup", 3), (40, 2, "few", 4)):
        x = (torch.rand(T, K, generator=g) - 0.5).half()
        x[t] = row
        idx = _routing(T, k, E, kind, seed)
        idx[t, 0], idx[t, 1] = 4, E - 1
        _, offsets, sorted_slot, position, active = _route(lib, idx, E)
        y = torch.empty(T * k, N, dtype=torch.float16, device=DEV)
        assert lib.eetq_w4a16_moe_gemm(_ptr(x.to(DEV)), _ptr(proc), _ptr(scales), _ptr(offsets), _ptr(sorted_slot), _ptr(active),
                                       _ptr(y), T, k, E, N, K, 1, 0, _stream()) == 0
        pos = position.view(T, k)[t].long()
        got.append(y[pos].clone())
        places.append(tuple(int(p - offsets[e]) for p, e in zip(pos, (4, E - 1))))
    torch.cuda.synchronize()
    assert max(p[1] for p in places) >= 16 and len(set(places)) > 2   # different places, some beyond the first row tile
    for other in got[1:]:
        assert torch.equal(other, got[0])


def _int8_stack_on_cpu(raw):
    """[E, K, N/2] raw int4 -> [E, K, N] int8 gfx950 tiles holding the same integers, built by the oracle"""
    import oracle
    return torch.from_numpy(np.stack([oracle.gfx950_pack(oracle.i4_values(r)) for r in raw.numpy()]))


@pytest.mark.parametrize("E,K,N", [(1, 128, 16), (3, 384, 64), (8, 512, 768)])
def test_expansion_equals_the_int8_stack_of_the_same_integers(lib, E, K, N):
    (raw, proc, _), (graw, gproc, _) = _stack4(E, K, N, seed=E + K)
    for r, p in ((raw, proc), (graw, gproc)):   # glu8 order survives: the columns are untouched
        dst = torch.full((E, K, N), 99, dtype=torch.int8, device=DEV)
        assert lib.eetq_expand_i4_to_i8(_ptr(p), _ptr(dst), p.numel(), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu(), _int8_stack_on_cpu(r))


PROMPT_SHAPES = {"mixtral-like": (8, 512, 384, 2), "qwen3-like": (128, 384, 384, 8)}   # E, H, I, k


@pytest.mark.parametrize("T", [64, 512])
@pytest.mark.parametrize("shape", list(PROMPT_SHAPES))
def test_prompt_path_equals_the_int8_chain_bit_for_bit(lib, shape, T):
    from eetq_amd.ops import quant_weights, w4_a16_moe, w4_a16_moe_path
    E, H, I, k = PROMPT_SHAPES[shape]
    torch.manual_seed(T + E)
    gu = _glu8_cols((torch.randn(E, H, 2 * I, device=DEV) * 1.5 / H ** 0.5).half())
    dn = (torch.randn(E, I, H, device=DEV) * 2.0 / I ** 0.5).half()
    gu_raw, gu_q, gu_s = quant_weights(gu, torch.quint4x2, True)
    dn_raw, dn_q, dn_s = quant_weights(dn, torch.quint4x2, True)
    gu8, dn8 = _int8_stack_on_cpu(gu_raw.cpu()).to(DEV), _int8_stack_on_cpu(dn_raw.cpu()).to(DEV)
    x = torch.randn(T, H, device=DEV).half()
    for kind in ("uniform", "sentinel", "one"):
        idx = _routing(T, k, E, kind, seed=T)
        wts = _router_weights(T, k, seed=T + 1)
        got = w4_a16_moe(x, idx, wts, gu_q, gu_s, dn_q, dn_s, path="expand")
        # the chain through the C ABI on the int8 stack
        S = T * k
        counts, offsets, sorted_slot, position, active = _route(lib, idx, E)
        tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
        inter = torch.empty(S, I, dtype=torch.float16, device=DEV)
        down = torch.empty(S, H, dtype=torch.float16, device=DEV)
        want = torch.empty(T, H, dtype=torch.float16, device=DEV)
        f = lib.eetq_w8a16_moe_gemm_tiled
        assert f(_ptr(x), _ptr(gu8), _ptr(gu_s), *tab, _ptr(inter), T, k, E, 2 * I, H, 1, 1, _stream()) == 0
        assert f(_ptr(inter), _ptr(dn8), _ptr(dn_s), *tab, _ptr(down), T, k, E, H, I, 0, 0, _stream()) == 0
        assert lib.eetq_moe_combine_f16(_ptr(down), _ptr(position), _ptr(wts), 1, _ptr(want), T, k, H, _stream()) == 0
        torch.cuda.synchronize()
        assert float(want.float().abs().max()) > 0.5
        assert torch.equal(got, want), kind
        # what the shape rule does on its own: the path it reports, bit for bit
        auto = w4_a16_moe_path(T, k, E, H, I)
        assert auto in ("expand", "decode")
        assert torch.equal(w4_a16_moe(x, idx, wts, gu_q, gu_s, dn_q, dn_s),
                           got if auto == "expand" else w4_a16_moe(x, idx, wts, gu_q, gu_s, dn_q, dn_s, path="decode")), kind
    if (E, k, T) == (8, 2, 512):
        assert w4_a16_moe_path(T, k, E, H, I) == "expand"


def test_named_expanded_path_refuses_shapes_the_tiled_kernel_cannot_take():
    from eetq_amd.ops import w4_a16_moe, w4_a16_moe_path
    _, q = _experts4(8, 256, 128, 2, seed=2)    # K = 256 and 128 < 320
    x = torch.randn(64, 256, device=DEV).half()
    idx = _routing(64, 2, 8, "uniform", seed=1)
    wts = _router_weights(64, 2, seed=1)
    stacks = (q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)
    assert w4_a16_moe_path(4096, 2, 8, 256, 128) == "decode"
    with pytest.raises(RuntimeError, match="expand"):
        w4_a16_moe(x, idx, wts, *stacks, path="expand")
    with pytest.raises(RuntimeError, match="path"):
        w4_a16_moe(x, idx, wts, *stacks, path="tiled")
    assert torch.equal(w4_a16_moe(x, idx, wts, *stacks), w4_a16_moe(x, idx, wts, *stacks, path="decode"))


@pytest.mark.parametrize("E,H,I,k", [(8, 256, 128, 2), (128, 128, 128, 8), (8, 512, 768, 2)])
@pytest.mark.parametrize("T", [1, 4, 16])
@pytest.mark.parametrize("kind", ["uniform", "one", "sentinel", "dup"])
def test_layer_against_float64_reference(E, H, I, k, T, kind):
    _, q = _experts4(E, H, I, k, seed=E + H)
    vals = _module_values(q)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, kind, seed=T)
    for wts in (_router_weights(T, k, seed=T + 1), _router_weights(T, k, seed=T + 2).half()):
        y = q(x, idx, wts)
        assert y.shape == (T, H) and y.dtype == torch.float16 and not y.requires_grad
        ref = _layer_ref64(x, idx, wts, vals, E)
        assert np.abs(ref.astype(np.float32)).max() > 0.25
        err = np.abs(y.cpu().numpy().astype(np.float32) - ref.astype(np.float32))
        assert _tier_a(y.cpu().numpy(), ref).all(), (float(err.max()), float(np.abs(ref).max()))
        assert torch.equal(q(x, idx, wts), y)   # two calls, the same bits
    # the bound has teeth: zeros and reversed router weights fail it
    assert not _tier_a(np.zeros_like(ref), ref).all()
    if kind != "dup":
        assert not _tier_a(_layer_ref64(x, idx, wts.flip(-1), vals, E), ref).all()


@pytest.mark.parametrize("E,H,I,k,T,path", [(8, 256, 128, 2, 16, "decode"), (8, 512, 384, 2, 512, "expand")])
def test_graph_replay_with_rewritten_routing_and_hidden(E, H, I, k, T, path):
    from eetq_amd.ops import w4_a16_moe_path
    assert w4_a16_moe_path(T, k, E, H, I) == path
    _, q = _experts4(E, H, I, k, seed=9)
    x = torch.randn(T, H, device=DEV).half()
    idx = _routing(T, k, E, "uniform", seed=1)
    wts = _router_weights(T, k, seed=2)
    assert torch.equal(q(x, idx, wts), q(x, idx, wts))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        q(x, idx, wts)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = q(x, idx, wts)
    for seed, kind in ((2, "uniform"), (3, "sentinel"), (4, "one"), (5, "dup")):
        idx.copy_(_routing(T, k, E, kind, seed=seed))
        wts.copy_(_router_weights(T, k, seed=seed))
        x.copy_(torch.randn(T, H, device=DEV).half())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, q(x, idx, wts)), kind


def test_state_dict_round_trip_is_bit_identical():
    from eetq_amd.modules.qlinear import W4A16Experts
    src, q = _experts4(16, 128, 128, 4, seed=3)
    sd = {n: t.clone() for n, t in q.state_dict().items()}
    assert set(sd) == {"gate_up_qweight", "gate_up_scales", "down_qweight", "down_scales"}
    assert all(torch.equal(sd[n], getattr(q, n)) for n in sd)   # the buffers as they are: no re-encoding
    fresh = W4A16Experts.from_experts(src, init_only=True)
    fresh.load_state_dict(sd)
    for T in (3, 20):
        x = (torch.rand(T, 128, device=DEV) - 0.5).half()
        idx = _routing(T, 4, 16, "random", seed=T)
        wts = torch.rand(T, 4, device=DEV).softmax(-1)
        assert torch.equal(fresh(x, idx, wts), q(x, idx, wts))


def _tiny4(which):
    from transformers import MixtralConfig, MixtralForCausalLM, Qwen3MoeConfig, Qwen3MoeForCausalLM
    torch.manual_seed(0)
    if which == "mixtral":
        cfg = MixtralConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=2, num_local_experts=8, num_experts_per_tok=2, vocab_size=512,
                            initializer_range=0.1)
        return MixtralForCausalLM(cfg).half().to(DEV).eval()
    cfg = Qwen3MoeConfig(hidden_size=128, intermediate_size=256, moe_intermediate_size=128, num_hidden_layers=2,
                         num_attention_heads=4, num_key_value_heads=2, num_experts=16, num_experts_per_tok=4, vocab_size=512,
                         decoder_sparse_step=1, mlp_only_layers=[], initializer_range=0.1)
    return Qwen3MoeForCausalLM(cfg).half().to(DEV).eval()


@pytest.mark.parametrize("which", ["mixtral", "qwen3_moe"])
def test_tiny_models_after_eet_quantize_expert_bits_4(which):
    from eetq_amd.modules.qlinear import W4A16Experts
    from eetq_amd.utils.quantizer import eet_quantize
    model = _tiny4(which)
    fp16_bytes = sum(p.numel() * 2 for n, p in model.named_parameters() if ".experts." in n)
    eet_quantize(model, experts=True, expert_bits=4)
    experts = [layer.mlp.experts for layer in model.model.layers]
    assert len(experts) == 2 and all(type(m) is W4A16Experts for m in experts)
    assert sum(b.numel() * b.element_size() for m in experts for b in m.buffers()) <= 0.27 * fp16_bytes
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, args, out, i=i: seen.setdefault(i, []).append((args, out)))
             for i, m in enumerate(experts)]
    ids = torch.randint(0, 512, (2, 24), generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        logits = model(ids).logits
    for h in hooks:
        h.remove()
    assert np.isfinite(logits.float().cpu().numpy()).all()
    for i, m in enumerate(experts):   # every experts module on the hidden states it actually received
        assert len(seen[i]) == 1
        (hidden, idx, wts), out = seen[i][0]
        assert hidden.shape == (48, 128) and out.shape == (48, 128)
        ref = _layer_ref64(hidden, idx, wts, _module_values(m), m.num_experts)
        err = np.abs(out.cpu().numpy().astype(np.float32) - ref.astype(np.float32))
        assert np.abs(ref.astype(np.float32)).max() > 0
        assert _tier_a(out.cpu().numpy(), ref).all(), (i, float(err.max()), float(np.abs(ref).max()))
    prompt = ids[:1, :10]
    gen = model.generate(prompt, max_new_tokens=16, do_sample=False, min_new_tokens=16)
    assert gen.shape == (1, 26)
    # state_dict() -> a fresh init_only model -> load_state_dict(): the same logits bit for bit
    fresh = _tiny4(which)
    eet_quantize(fresh, init_only=True, experts=True, expert_bits=4)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(ids).logits, logits)
    assert torch.equal(fresh.generate(prompt, max_new_tokens=16, do_sample=False, min_new_tokens=16), gen)
