"""fp32 accumulation and ONE rounding in the routed mixture-of-experts kernels -- bit for bit, with no tolerance anywhere in this file.
The inputs (tests/moe_exact_cases.py on tests/exact_cases.py) make every product an integer number of quanta and keep the sum of
their magnitudes below 2^24 quanta, so every partial sum in every order is an fp32 value: whatever a kernel's waves, stages, tails,
rings or reduction through LDS, its accumulator holds the exact sum and every live row must equal fp16(exact sum) as a number; every
row at or past offsets[E] must still hold what the buffer was filled with.  Every expert has its own codes and scales, the routing
has experts with 0, 1, 15, 16, 17 and 33 rows, a slot on the id E and one on -1, and the contiguous runs read NaN where no row is.
tests/test_moe_exact_cases_cpu.py asserts the condition on every element, and shows what tier A made of the same faults: it accepts
every early rounding (fp16 wave partials among them) and one lost product of a 1-row expert, and would have seen a lost k tile had
it run these K.

The routing tables come from eetq_moe_route and must equal the NumPy tables the references are laid out by.  The glu8 write-out is held
to eetq_silu_mul_glu8_f16 applied on the device to the uploaded exact reference of the glu8-ordered stack's plain projection, bit
for bit.  A failure names the number of wrong elements, the first with both values and the distance in quanta, the experts, the
16-row groups and the 16-column tile rows that hold them, and the case's (waves, depth) and k tiles per wave.

The (waves, depth) and tiles per wave of a decode case rest on the RESTATED plan rule (moe_exact_cases.plan): the library has no
host query for the MoE plan, so that each K runs the instantiation it is listed for is unverified here; exactness does not depend on it.

form (cases)                                                                                              result on an MI355X
  decode kernel, int8: K = 64 .. 2112 on 1 x 1, 4 x 2 and 8 x 2; gather, contiguous, glu8 of each             (9)          exact
  decode kernel, int4: K = 128 .. 9088 on 1 x 1, 2 x 1, 4 x 1 and 8 x 2; gather, contiguous, glu8 of each     (10)         exact
  tiled prompt kernel, int8: K = 320, 384, 448 (5, 6, 7 K steps), gather and contiguous                      (3)          exact
  tiled prompt kernel, int4: K = 384, 512, 640 at tile_j = 0, 1, 2, gather and contiguous                    (3)          exact
  int4 tiled kernel at K = 256: the quiet refusal, output untouched                                           (3)          refused
  grouped input gradient: int8 (320, 272), int4 (384, 272)                                                    (2)          exact
  combine: T 1 / 5, k 1 / 2 / 8, H 8 / 2040 / 2048 / 2056, fp32 and fp16 weights                              (48)         exact
All 78 tests pass on the device: no kernel and no plan rule had to change.  Wall time of the file on an MI355X: 3.2 s (the slowest:
the first case 0.4 s with the module's start-up, the first tiled case 0.15 s, every other test under 0.1 s).
"""
import ctypes

import numpy as np
import pytest
import torch

import moe_exact_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_UNSUPPORTED = -3


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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(lib, route):
    """eetq_moe_route's tables of the route's ids, which must be the NumPy tables the reference is laid out by: (offsets, sorted_slot, active)"""
    from test_gpu_moe import _route
    got = _route(lib, _dev(route.idx), route.E)
    torch.cuda.synchronize()
    for name, g, want in zip(("counts", "offsets", "sorted_slot", "position", "active"), got,
                             (route.counts, route.offsets, route.sorted_slot, route.position, route.active)):
        assert np.array_equal(g.cpu().numpy(), want), name
    return got[1], got[2], got[4]


@pytest.fixture(scope="module")
def decode_route(lib):
    route = mc.decode_routing()
    return route, _tables(lib, route)


def _stack(oracle, rp, glu8=False):
    """the experts' weights packed with the oracle: ([E, K, N] int8 or [E, K, N / 2] int4 tiles, [E, N] scales) on the GPU"""
    from test_gpu_moe_int4 import _glu8_cols
    packed, scales = [], []
    for w in rp.w:
        q, s = w.q, w.s
        if glu8:
            q, s = _glu8_cols(torch.from_numpy(q)).numpy(), _glu8_cols(torch.from_numpy(s)).numpy()
        packed.append(oracle.gfx950_pack(q) if rp.case.bits == 8 else oracle.gfx950_pack_i4(oracle.i4_from_values(q)))
        scales.append(s)
    return _dev(np.stack(packed)), _dev(np.stack(scales))


def _explain(name, rp, got, want, plan=None, quantum=None):
    r = rp.route
    quantum = rp.quantum() if quantum is None else quantum
    bad = np.argwhere(~(got.astype(np.float32) == want.astype(np.float32)))
    m, n = bad[0]
    owner = r.expert_of_row()
    experts = sorted(set(owner[bad[:, 0]].tolist()))
    groups = sorted({(int(owner[p]), int((p - r.offsets[owner[p]]) // 16)) if owner[p] >= 0 else (-1, int(p)) for p in bad[:, 0]})
    dq = (float(got[m, n]) - float(want[m, n])) / quantum[m, n]
    return ("%s [%s]: %d of %d elements differ from fp16(exact sum); first at row %d (expert %d, its row %d) column %d: device %r, reference %r, %+.2f quanta "
            "of %g; experts %s (-1: rows at or past offsets[E]); 16-row groups (expert, group) %s; 16-column tile rows %s (of %d); plan %s"
            % (name, rp.case.form, len(bad), got.size, m, owner[m], m - (r.offsets[owner[m]] if owner[m] >= 0 else 0), n, float(got[m, n]), float(want[m, n]), dq,
               quantum[m, n], experts, groups[:16], sorted(set((bad[:, 1] // 16).tolist()))[:20], (got.shape[1] + 15) // 16,
               plan or "(none: not the decode kernel)"))


def _check(name, rp, got, want, plan=None, quantum=None):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float16, name
    if not np.array_equal(got.astype(np.float32), want.astype(np.float32)):       # NaN equals nothing: a NaN anywhere fails
        pytest.fail(_explain(name, rp, got, want, plan, quantum))


def _poison(rows, cols):
    return torch.full((rows, cols), mc.POISON, dtype=torch.float16, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- decode kernel
@pytest.mark.parametrize("dc", mc.DECODE_CASES, ids=lambda d: d.id)
def test_decode_kernel(lib, oracle, decode_route, dc):
    from test_gpu_moe_int4 import _glu8_cols
    route, tab = decode_route
    rp = mc.Routed(dc.case, route)
    assert rp.bound() < mc.LIMIT, dc.id
    want = rp.reference()
    plan = "%d x %d, k tiles per wave %s" % (dc.waves, dc.depth, dc.tiles)
    f = lib.eetq_w8a16_moe_gemm if dc.bits == 8 else lib.eetq_w4a16_moe_gemm
    T, k, E, N, K, S = route.T, route.k, route.E, mc.N, dc.K, route.S
    tabs = tuple(_ptr(t) for t in tab)
    w, s = _stack(oracle, rp)
    gw, gs = _stack(oracle, rp, glu8=True)
    xs = {1: _dev(mc.as_x(rp.i)), 0: _dev(rp.sorted_x())}
    assert bool(xs[0][route.used:].isnan().all()) and xs[1].shape == (T, K) and xs[0].shape == (S, K)
    # what the gated write-out must be: eetq_silu_mul_glu8_f16 on the exact reference of the glu8-ordered stack's plain projection
    want_g = _glu8_cols(torch.from_numpy(want + np.float16(0)))
    gated, want_gd = _poison(S, N // 2), want_g.to(DEV)
    assert lib.eetq_silu_mul_glu8_f16(_ptr(want_gd), _ptr(gated), S, N // 2, _stream()) == 0
    for gather in (1, 0):
        y, yg, g = _poison(S, N), _poison(S, N), _poison(S, N // 2)
        assert f(_ptr(xs[gather]), _ptr(w), _ptr(s), *tabs, _ptr(y), T, k, E, N, K, gather, 0, _stream()) == 0
        assert f(_ptr(xs[gather]), _ptr(gw), _ptr(gs), *tabs, _ptr(yg), T, k, E, N, K, gather, 0, _stream()) == 0
        assert f(_ptr(xs[gather]), _ptr(gw), _ptr(gs), *tabs, _ptr(g), T, k, E, N, K, gather, 1, _stream()) == 0
        torch.cuda.synchronize()
        _check("%s, gather = %d" % (dc.id, gather), rp, y, want, plan)
        _check("%s, gather = %d, glu8-ordered stack" % (dc.id, gather), rp, yg, want_g.numpy(), plan,
               _glu8_cols(torch.from_numpy(rp.quantum())).numpy())
        assert torch.equal(g[:route.used], gated[:route.used]), (dc.id, gather, plan, int((g[:route.used] != gated[:route.used]).sum()))
        assert bool((g[route.used:] == mc.POISON).all()), (dc.id, gather)


# ---------------------------------------------------------------------------------------------------------------- tiled prompt kernels
@pytest.mark.parametrize("case", mc.TILED_CASES, ids=lambda c: c.id)
def test_tiled_prompt_kernel(lib, oracle, case):
    from test_gpu_moe_prompt import _prompt_routing
    idx = _prompt_routing(385, 1, mc.E, "straddle", seed=case.K)
    route = mc.straddle_routing(idx.cpu().numpy())
    tab = _tables(lib, route)             # held to the end of the test: the kernels read them
    tabs = tuple(_ptr(t) for t in tab)
    rp = mc.Routed(case, route)
    assert rp.bound() < mc.LIMIT, case.id
    want = rp.reference()
    T, k, E, N, K, S = route.T, route.k, route.E, case.N, case.K, route.S
    w, s = _stack(oracle, rp)
    xs = {1: _dev(mc.as_x(rp.i)), 0: _dev(rp.sorted_x())}
    for gather in (1, 0):
        if case.bits == 8:
            assert lib.eetq_w8a16_moe_gemm_tiled_supported(T, k, E, N, K, gather) == 1
            y = _poison(S, N)
            assert lib.eetq_w8a16_moe_gemm_tiled(_ptr(xs[gather]), _ptr(w), _ptr(s), *tabs, _ptr(y), T, k, E, N, K, gather, 0, _stream()) == 0
            torch.cuda.synchronize()
            _check("%s, gather = %d" % (case.id, gather), rp, y, want)
            continue
        assert lib.eetq_w4a16_moe_gemm_tiled_supported(T, k, E, N, K, gather) == 1
        for tile_j in (0, 1, 2):
            y = _poison(S, N)
            assert lib.eetq_w4a16_moe_gemm_tiled(_ptr(xs[gather]), _ptr(w), _ptr(s), *tabs, _ptr(y), T, k, E, N, K, gather, 0, tile_j, _stream()) == 0
            torch.cuda.synchronize()
            _check("%s, gather = %d, tile_j = %d" % (case.id, gather, tile_j), rp, y, want)


@pytest.mark.parametrize("gather,glu8", [(1, 0), (1, 1), (0, 0)])
def test_int4_k_below_the_ring_minimum_is_quietly_unsupported(lib, gather, glu8):
    from test_gpu_moe import _route, _routing
    from test_gpu_moe_int4 import _stack4
    T, k, E, N, K = 64, 2, 8, 256, 256   # two int4 tiles = four K steps < the six the drain needs
    (_, proc, scales), _ = _stack4(E, K, N, seed=1)
    _, offsets, sorted_slot, _, active = _route(lib, _routing(T, k, E, "uniform", seed=1), E)
    x = torch.zeros(T * k, K, dtype=torch.float16, device=DEV)
    assert lib.eetq_w4a16_moe_gemm_tiled_supported(T, k, E, N, K, gather) == 0
    for tile_j in (0, 1, 2):
        y = _poison(T * k, N)
        rc = lib.eetq_w4a16_moe_gemm_tiled(_ptr(x), _ptr(proc), _ptr(scales), _ptr(offsets), _ptr(sorted_slot), _ptr(active), _ptr(y),
                                           T, k, E, N, K, gather, glu8, tile_j, _stream())
        assert rc == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert bool((y == mc.POISON).all())   # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- grouped gradient
@pytest.mark.parametrize("case", mc.GRAD_CASES, ids=lambda c: c.id)
def test_grouped_input_gradient(lib, oracle, decode_route, case):
    route, (offsets, _, active) = decode_route
    rp = mc.Routed(case, route)
    assert rp.bound() < mc.LIMIT, case.id
    want = rp.reference()
    w, s = _stack(oracle, rp)
    dy = mc.as_x(rp.i)
    dy[route.used:] = np.nan              # rows no expert owns: nothing may read them into a live row
    dyd, dx = _dev(dy), _poison(route.S, case.K)
    f = lib.eetq_w8a16_moe_gemm_t if case.bits == 8 else lib.eetq_w4a16_moe_gemm_t
    assert f(_ptr(dyd), _ptr(w), _ptr(s), _ptr(offsets), _ptr(active), _ptr(dx), route.T, route.k, route.E, case.N, case.K, _stream()) == 0
    torch.cuda.synchronize()
    _check(case.id, rp, dx, want)


# ---------------------------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("c", mc.COMBINE_CASES, ids=lambda c: c.id)
def test_combine(lib, c):
    p = mc.Combine(c)
    assert p.bound() < 2 ** 18
    want = p.reference()
    y, pos, w = _dev(p.y), _dev(p.position), _dev(p.w)
    assert w.dtype == (torch.float32 if c.wdtype == "f32" else torch.float16) and bool(y.isnan().any())
    out = _poison(c.T, c.H)
    assert lib.eetq_moe_combine_f16(_ptr(y), _ptr(pos), _ptr(w), 1 if c.wdtype == "f32" else 0, _ptr(out), c.T, c.k, c.H, _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), c.id
    if not np.array_equal(got.astype(np.float32), want.astype(np.float32)):
        bad = np.argwhere(got.astype(np.float32) != want.astype(np.float32))
        t, h = bad[0]
        pytest.fail("%s: %d of %d elements differ from fp16(sum_j fp32(y) fp32(w)); first at token %d column %d: device %r, reference %r, %+.2f quanta of 2^-10; "
                    "tokens %s, positions of the first %s, weights (sixteenths) %s"
                    % (c.id, len(bad), got.size, t, h, float(got[t, h]), float(want[t, h]), (float(got[t, h]) - float(want[t, h])) / p.quantum,
                       sorted(set(bad[:, 0].tolist())), p.position.reshape(c.T, c.k)[t].tolist(), p.m[t].tolist()))
    if c.T > 1:
        assert not got[2].any()           # the token whose slots are all -1
