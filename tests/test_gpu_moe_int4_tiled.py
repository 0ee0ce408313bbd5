"""The grouped tiled MFMA kernel on int4 expert stacks (path "direct"): eetq_w4a16_moe_gemm_tiled against the
shipped prompt path -- eetq_expand_i4_to_i8 followed by eetq_w8a16_moe_gemm_tiled on the same tables -- BIT FOR BIT (torch.equal,
no tolerance) at both tile shapes and the launcher's own choice, since both apply fp16(q s) with one rounding and add each output's
products in the same k order whatever the column blocking.  One case is also held to the oracle (tier A, |err| <= 1e-3 max|ref| +
2e-3 |ref|) so that a defect shared with the expanded path cannot pass.  Then the operators (path="direct" against path="expand"
and the float64 layer reference), the missing expansion buffer, graph replay, and a tiny Mixtral with the module switch.

Shapes of the sweep: K = 384 (six K steps: the drain only), 512 (one steady pair), 768 (the six-slot ring wraps), 1152 (nine int4
tiles per column tile: an odd count); N = 144 (nine column tiles: odd, so the last half-wave DMA is clamped), 208 (ragged last
tile at 64 and at 128 columns), 256 (even).  Rows per expert 0, 1, 127, 128, 129 and 257 in one call."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_moe import _route, _router_weights, _routing, _tier_a
from test_gpu_moe_int4 import _experts4, _glu8_cols, _layer_ref64, _module_values, _stack4

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


def _ids_with_counts(counts, T, k, E, seed):
    """[T, k] expert ids with exactly counts[e] slots on expert e, the remaining slots on the sentinel E (no row), shuffled"""
    flat = torch.cat([torch.full((c,), e, dtype=torch.long) for e, c in enumerate(counts)] +
                     [torch.full((T * k - sum(counts),), E, dtype=torch.long)])
    flat = flat[torch.randperm(T * k, generator=torch.Generator().manual_seed(seed))]
    return flat.view(T, k).to(DEV)


E_SWEEP = 8
# (T, k, counts): every row-count edge of a 128-row tile in one call; a single active expert; fewer slots than experts
ROUTINGS = {"edges": (330, 2, [0, 1, 127, 128, 129, 257, 10, 0]),
            "single": (20, 2, [0, 0, 0, 40, 0, 0, 0, 0]),
            "few-slots": (3, 2, [0, 2, 0, 0, 1, 0, 0, 3])}


@pytest.fixture(scope="module")
def tables(lib):
    out = {}
    for name, (T, k, counts) in ROUTINGS.items():
        idx = _ids_with_counts(counts, T, k, E_SWEEP, seed=T)
        got, offsets, sorted_slot, position, active = _route(lib, idx, E_SWEEP)
        torch.cuda.synchronize()
        assert got.cpu().tolist() == counts
        out[name] = (T, k, offsets, sorted_slot, active)
    assert ROUTINGS["few-slots"][0] * ROUTINGS["few-slots"][1] < E_SWEEP
    return out


def _expanded(lib, proc, E, K, N):
    w8 = torch.empty(E, K, N, dtype=torch.int8, device=DEV)
    assert lib.eetq_expand_i4_to_i8(_ptr(proc), _ptr(w8), proc.numel(), _stream()) == 0
    return w8


def _inputs(T, k, K, offsets, sorted_slot, gather, seed):
    """x for the gathering form ([T, K]) or the contiguous one ([T k, K]: the gathered rows in sorted order, NaN past offsets[E])"""
    x = (torch.rand(T, K, generator=torch.Generator().manual_seed(seed)) - 0.5).half()
    if gather:
        return x, x.to(DEV)
    used = int(offsets[-1])
    rows = torch.cat([x[sorted_slot[:used].long().cpu() // k], torch.full((T * k - used, K), float("nan"), dtype=torch.float16)])
    return x, rows.to(DEV)


@pytest.mark.parametrize("N", [144, 208, 256])
@pytest.mark.parametrize("K", [384, 512, 768, 1152])
def test_direct_equals_expansion_plus_int8_tile_bit_for_bit(lib, tables, K, N):
    import oracle
    E = E_SWEEP
    (raw, proc, scales), (_, gproc, gscales) = _stack4(E, K, N, seed=K + N)
    f4, f8 = lib.eetq_w4a16_moe_gemm_tiled, lib.eetq_w8a16_moe_gemm_tiled
    assert lib.eetq_w4a16_moe_gemm_tiled_supported(330, 2, E, N, K, 1) == 1
    for name, (T, k, offsets, sorted_slot, active) in tables.items():
        S, used = T * k, int(offsets[-1])
        tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
        for gather in (1, 0):
            x_cpu, x = _inputs(T, k, K, offsets, sorted_slot, gather, seed=K + T)
            for glu8 in ((0, 1) if N == 256 else (0,)):
                w4, sc = (gproc, gscales) if glu8 else (proc, scales)
                cols = N // 2 if glu8 else N
                want = torch.full((S, cols), POISON, dtype=torch.float16, device=DEV)
                w8 = _expanded(lib, w4, E, K, N)
                assert f8(_ptr(x), _ptr(w8), _ptr(sc), *tab, _ptr(want), T, k, E, N, K, gather, glu8, _stream()) == 0
                torch.cuda.synchronize()
                assert not bool((want[:used] == POISON).any()) and not bool(want[:used].isnan().any())
                for tile_j in (0, 1, 2):
                    got = torch.full((S, cols), POISON, dtype=torch.float16, device=DEV)
                    assert f4(_ptr(x), _ptr(w4), _ptr(sc), *tab, _ptr(got), T, k, E, N, K, gather, glu8, tile_j, _stream()) == 0
                    torch.cuda.synchronize()
                    assert bool((got[used:] == POISON).all()), (name, gather, glu8, tile_j)     # untouched rows
                    assert torch.equal(got, want), (name, gather, glu8, tile_j,
                                                    int((got != want).sum()), float((got.float() - want.float()).abs().max()))
            if (K, N, name, gather) == (512, 208, "edges", 1):   # the independent check: the oracle per expert, tier A
                got = torch.full((S, N), POISON, dtype=torch.float16, device=DEV)
                assert f4(_ptr(x), _ptr(proc), _ptr(scales), *tab, _ptr(got), T, k, E, N, K, 1, 0, 0, _stream()) == 0
                torch.cuda.synchronize()
                off, slots = offsets.cpu().numpy(), sorted_slot.cpu().numpy()
                for e in range(E):
                    rows = slice(off[e], off[e + 1])
                    if off[e + 1] == off[e]:
                        continue
                    vals = oracle.i4_values(oracle.gfx950_unpack_i4(proc[e].cpu().numpy()))
                    assert np.array_equal(vals, oracle.i4_values(raw[e].numpy()))
                    ref = oracle.w8a16_gemm(x_cpu.numpy()[slots[rows] // k], vals, scales[e].cpu().numpy())
                    y = got[rows].cpu().numpy()
                    assert np.abs(ref.astype(np.float32)).max() > 0.1
                    assert _tier_a(y, ref).all(), (e, float(np.abs(y.astype(np.float32) - ref.astype(np.float32)).max()))
                    assert not _tier_a(np.zeros_like(ref), ref).all()


def test_tile_j_0_takes_the_wide_tile_where_the_launchers_rule_does(lib):
    """E = 8 with 16 rows each, N = 4096, K = 384: 8 row tiles x 32 wide column tiles fill 256 CUs in one round, 64 narrow ones need
    two -- the int8 launcher's rule picks the 128 x 128 tile, and tile_j = 0 must follow it"""
    E, K, N, T, k = 8, 384, 4096, 64, 2
    (_, proc, scales), _ = _stack4(E, K, N, seed=11)
    idx = _ids_with_counts([16] * E, T, k, E, seed=3)
    counts, offsets, sorted_slot, _, active = _route(lib, idx, E)
    tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
    x = (torch.rand(T, K, generator=torch.Generator().manual_seed(1)) - 0.5).half().to(DEV)
    want = torch.full((T * k, N), POISON, dtype=torch.float16, device=DEV)
    w8 = _expanded(lib, proc, E, K, N)
    assert lib.eetq_w8a16_moe_gemm_tiled(_ptr(x), _ptr(w8), _ptr(scales), *tab, _ptr(want), T, k, E, N, K, 1, 0, _stream()) == 0
    for tile_j in (0, 2, 1):
        got = torch.full((T * k, N), POISON, dtype=torch.float16, device=DEV)
        assert lib.eetq_w4a16_moe_gemm_tiled(_ptr(x), _ptr(proc), _ptr(scales), *tab, _ptr(got), T, k, E, N, K, 1, 0, tile_j,
                                             _stream()) == 0
        torch.cuda.synchronize()
        assert int(counts.min()) >= 1 and not bool((got == POISON).any())
        assert torch.equal(got, want), tile_j


def test_result_does_not_depend_on_where_the_operands_are_allocated(lib, tables):
    E, K, N = E_SWEEP, 768, 208
    (_, proc, scales), _ = _stack4(E, K, N, seed=5)
    T, k, offsets, sorted_slot, active = tables["edges"]
    tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
    _, x = _inputs(T, k, K, offsets, sorted_slot, 1, seed=2)
    outs = []
    for w_shift, x_shift in ((0, 0), (1024 + 16, 48)):   # bytes; 16-byte aligned as the entry demands
        wbuf = torch.zeros(proc.numel() + w_shift, dtype=torch.int8, device=DEV)
        xbuf = torch.zeros(x.numel() + x_shift // 2, dtype=torch.float16, device=DEV)
        w = wbuf[w_shift:].view(proc.shape).copy_(proc)
        xx = xbuf[x_shift // 2:].view(x.shape).copy_(x)
        assert w.data_ptr() % 16 == 0 and xx.data_ptr() % 16 == 0
        y = torch.full((T * k, N), POISON, dtype=torch.float16, device=DEV)
        assert lib.eetq_w4a16_moe_gemm_tiled(_ptr(xx), _ptr(w), _ptr(scales), *tab, _ptr(y), T, k, E, N, K, 1, 0, 0, _stream()) == 0
        torch.cuda.synchronize()
        outs.append(y)
    assert torch.equal(outs[0], outs[1]) and not bool((outs[0][:int(offsets[-1])] == POISON).any())


LAYER_SHAPES = {"mixtral-like": (8, 512, 384, 2), "qwen3-like": (128, 512, 384, 8)}   # E, H, I, k


@pytest.fixture(scope="module")
def layers():
    out = {}
    for name, (E, H, I, k) in LAYER_SHAPES.items():
        _, q = _experts4(E, H, I, k, seed=E + H)
        out[name] = (q, _module_values(q))
    return out


@pytest.mark.parametrize("T", [64, 512])
@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
def test_op_direct_equals_expand_bit_for_bit_and_the_float64_layer(layers, shape, T):
    from eetq_amd.ops import w4_a16_moe, w4_a16_moe_direct_supported
    E, H, I, k = LAYER_SHAPES[shape]
    q, vals = layers[shape]
    assert w4_a16_moe_direct_supported(T, k, E, H, I)
    stacks = (q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)
    x = torch.randn(T, H, device=DEV, generator=torch.Generator(DEV).manual_seed(T)).half()
    for kind in ("uniform", "sentinel", "one"):
        idx, wts = _routing(T, k, E, kind, seed=T), _router_weights(T, k, seed=T + 1)
        got = w4_a16_moe(x, idx, wts, *stacks, path="direct")
        assert torch.equal(got, w4_a16_moe(x, idx, wts, *stacks, path="expand")), kind
        assert torch.equal(got, w4_a16_moe(x, idx, wts, *stacks, path="direct")), kind
    # tier A against the float64 layer (a token's output depends on its own row and routing only: the first 64 tokens)
    n = 64
    ref = _layer_ref64(x[:n], idx[:n], wts[:n], vals, E)
    y = got[:n].cpu().numpy()
    assert np.abs(ref.astype(np.float32)).max() > 0.25
    assert _tier_a(y, ref).all(), float(np.abs(y.astype(np.float32) - ref.astype(np.float32)).max())
    assert not _tier_a(np.zeros_like(ref), ref).all()


def test_named_direct_path_refuses_shapes_the_kernel_cannot_take():
    from eetq_amd.ops import w4_a16_moe, w4_a16_moe_direct_supported
    _, q = _experts4(8, 128, 128, 2, seed=2)
    x = torch.randn(64, 128, device=DEV).half()
    idx, wts = _routing(64, 2, 8, "uniform", seed=1), _router_weights(64, 2, seed=1)
    stacks = (q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)
    assert not w4_a16_moe_direct_supported(64, 2, 8, 128, 128)
    with pytest.raises(RuntimeError, match=r"path='direct' needs .*384"):
        w4_a16_moe(x, idx, wts, *stacks, path="direct")
    with pytest.raises(RuntimeError, match=r"path must be 'auto', 'decode' or 'expand'.*'direct'"):
        w4_a16_moe(x, idx, wts, *stacks, path="tiled")


def test_block_op_direct_equals_expand(layers):
    from eetq_amd.ops import w4_a16_moe_block
    E, H, I, k = LAYER_SHAPES["mixtral-like"]
    q, _ = layers["mixtral-like"]
    g = torch.Generator(DEV).manual_seed(4)
    router = (torch.randn(E, H, device=DEV, generator=g) * 0.1).half()
    x = torch.randn(96, H, device=DEV, generator=g).half()
    args = (x, router, k, True, torch.float32, q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)
    got = w4_a16_moe_block(*args, path="direct")
    assert float(got.float().abs().max()) > 0.1
    assert torch.equal(got, w4_a16_moe_block(*args, path="expand"))


def test_direct_allocates_no_expanded_stack(layers):
    from eetq_amd.ops import w4_a16_moe
    E, H, I, k = LAYER_SHAPES["mixtral-like"]
    q, _ = layers["mixtral-like"]
    stacks = (q.gate_up_qweight, q.gate_up_scales, q.down_qweight, q.down_scales)
    T = 32
    x = torch.randn(T, H, device=DEV).half()
    idx, wts = _routing(T, k, E, "uniform", seed=1), _router_weights(T, k, seed=2)
    peaks = {}
    for path in ("direct", "expand"):
        w4_a16_moe(x, idx, wts, *stacks, path=path)   # warm: one-off allocations of the library and the allocator's pools
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = w4_a16_moe(x, idx, wts, *stacks, path=path)
        torch.cuda.synchronize()
        peaks[path] = torch.cuda.max_memory_allocated() - before
        del out
    assert peaks["direct"] < E * H * 2 * I, peaks
    assert peaks["expand"] >= E * H * 2 * I, peaks   # the measure sees the buffer where there is one


def test_graph_replay_of_the_direct_layer():
    E, H, I, k, T = 8, 512, 384, 2, 64
    _, q = _experts4(E, H, I, k, seed=9)
    q.prompt_path = "direct"
    assert q.op_path(T, k) == "direct"
    x = torch.randn(T, H, device=DEV).half()
    idx, wts = _routing(T, k, E, "uniform", seed=1), _router_weights(T, k, seed=2)
    assert torch.equal(q(x, idx, wts), q(x, idx, wts))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        q(x, idx, wts)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = q(x, idx, wts)
    for seed, kind in ((3, "sentinel"), (4, "one"), (5, "dup")):
        idx.copy_(_routing(T, k, E, kind, seed=seed))
        wts.copy_(_router_weights(T, k, seed=seed))
        x.copy_(torch.randn(T, H, device=DEV).half())
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, q(x, idx, wts)), kind


def _tiny_mixtral():
    """one decoder layer: the comparison against the decode kernel stays on the experts (a second layer's router can flip a choice
    on a last-bit difference, which no tolerance on logits covers)"""
    from transformers import MixtralConfig, MixtralForCausalLM
    torch.manual_seed(0)
    cfg = MixtralConfig(hidden_size=512, intermediate_size=384, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                        num_local_experts=8, num_experts_per_tok=2, vocab_size=512, initializer_range=0.1)
    return MixtralForCausalLM(cfg).half().to(DEV).eval()


def test_tiny_mixtral_with_the_module_switch(monkeypatch):
    from eetq_amd import ops
    from eetq_amd.modules import qlinear
    from eetq_amd.modules.qlinear import W4A16Experts
    from eetq_amd.utils.quantizer import eet_quantize
    default, direct = _tiny_mixtral(), _tiny_mixtral()
    eet_quantize(default, experts=True, expert_bits=4)
    eet_quantize(direct, experts=True, expert_bits=4, expert_prompt_path="direct")
    ex_default, ex_direct = default.model.layers[0].mlp.experts, direct.model.layers[0].mlp.experts
    assert type(ex_direct) is W4A16Experts and ex_direct.prompt_path == "direct" and ex_default.prompt_path == "auto"
    assert all(torch.equal(a, b) for a, b in zip(default.state_dict().values(), direct.state_dict().values()))
    ids = torch.randint(0, 512, (1, 64), generator=torch.Generator().manual_seed(1)).to(DEV)
    paths, seen = [], []
    real = qlinear.w4_a16_moe

    def spy(*args):
        paths.append(args[7])
        return real(*args)
    monkeypatch.setattr(qlinear, "w4_a16_moe", spy)
    hook = ex_default.register_forward_hook(lambda mod, args, out: seen.append((args, out)))
    with torch.no_grad():
        logits_direct = direct(ids).logits
        logits_default = default(ids).logits
    hook.remove()
    assert paths == ["direct", "auto"]
    # the default setting is the parent's call: the op without a path, on what the module received, bit for bit
    (hidden, idx, wts), out = seen[0]
    assert hidden.shape == (64, 512)
    stacks = (ex_default.gate_up_qweight, ex_default.gate_up_scales, ex_default.down_qweight, ex_default.down_scales)
    assert torch.equal(out, ops.w4_a16_moe(hidden, idx, wts, *stacks))
    # the same model with the op forced onto the expanded path: equal logits
    monkeypatch.setattr(qlinear, "w4_a16_moe", lambda *args: real(*args[:7], "expand"))
    with torch.no_grad():
        logits_expand = default(ids).logits
    assert np.isfinite(logits_direct.float().cpu().numpy()).all()
    assert torch.equal(logits_direct, logits_expand)
    # and against what the default rule runs here, the decode kernel (16 rows per expert: below its seam of 64): tier A
    assert ops.w4_a16_moe_path(64, 2, 8, 512, 384) == "decode"
    assert _tier_a(logits_direct[0].cpu().numpy(), logits_default[0].cpu().numpy()).all()
