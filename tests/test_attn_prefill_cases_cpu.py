"""The inputs of tests/test_gpu_attn_prefill_edges.py proved before the kernel sees them (tests/attn_cases.py): the 200-unit
gaps of the staircase and of the pairing families, the census's sensitivity to one dropped or doubled row, the ramp's rising
block maxima, the float64 reference itself, and the reach of the shape table.  A NumPy emulation of the kernel's arithmetic
(64-key blocks, fp32 scores in the exp2 domain, running maximum and sum, fp16-rounded probabilities for the value product,
fp32 accumulation, multiplication by the fp32 reciprocal, the per-wave `active` and `edge` decisions) goes through the very
drivers the GPU test uses and must pass them; eight mutants of it must each fail one.  No GPU."""
import numpy as np
import pytest

import attn_cases as ac
import test_gpu_attn_prefill_edges as edges

LOG2E = np.float32(1.4426950408889634)
P_SHIFT = np.float32(12.0)   # the kernel's kPfPShift; 0 is the arithmetic before it (test_unshifted_probabilities_miss_the_random_bound)
TABLE = [(r, i, D) for r in sorted(edges.ROWS) if r != 7 for i in range(len(edges.ROWS[r])) for D in edges.DIMS]
TABLE_IDS = ["row%d.%d-D%d" % t for t in TABLE]


def emulate(q, k, v, keys, koff, scale, mutant=None, shift=P_SHIFT):
    """The kernel's arithmetic on NumPy arrays: q [B, T, H, D], k, v [B, Hkv, S, D] fp16 -> fp16 [B, T, H, D].  Rows at and
    beyond `keys` read as zeros (the buffer descriptor's range).  mutant: (name, argument) or None."""
    name, arg = mutant if mutant else (None, None)
    B, T, H, D = q.shape
    Hkv = k.shape[1]
    koff = keys - T if koff is None else koff
    c = np.float32(np.float32(D ** -0.5 if scale is None else scale) * LOG2E)
    hk = np.arange(H) % Hkv if name == "kv_head_modulo" else np.arange(H) // (H // Hkv)
    nb_all = -(-keys // 64)
    kk = np.zeros((B, Hkv, nb_all * 64, D), dtype=np.float32)
    vv = np.zeros_like(kk)
    kk[:, :, :keys], vv[:, :, :keys] = k[:, :, :keys], v[:, :, :keys]
    kk, vv = kk[:, hk], vv[:, hk]                                             # [B, H, rows, D]
    qf = q.astype(np.float32).transpose(0, 2, 1, 3)                           # [B, H, T, D]
    t = np.arange(T)
    q0, w0 = (t // 128) * 128, (t // 32) * 32                                 # the row's query block and wave starts
    kend = np.minimum(keys, q0 + 128 + koff)
    nblk = np.where(kend > 0, -(-kend // 64), 0)
    m = np.full((B, H, T), -np.inf, dtype=np.float32)
    l = np.zeros((B, H, T), dtype=np.float32)
    o = np.zeros((B, H, T, D), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(nb_all):
            key0 = j * 64
            key = key0 + np.arange(64)
            run = (j < nblk) & (key0 <= w0 + 31 + koff)                       # the workgroup's loop, the wave's `active`
            if not run.any():
                continue
            edge = (key0 + 63 > w0 + koff) | (key0 + 64 > keys)
            if name == "edge_from_last_row":                                  # the wave's LAST row decides: diagonal blocks unmasked
                edge = (key0 + 63 > w0 + 31 + koff) | (key0 + 64 > keys)
            lim = (t + koff)[:, None]
            valid = key[None, :] < lim if name == "mask_lt" else key[None, :] <= lim + (1 if name == "mask_plus_one" else 0)
            valid = valid & (key[None, :] < keys)
            masked = edge[:, None] & ~valid                                   # [T, 64]
            if name == "drop_key":                                            # the key never reaches the softmax
                masked = masked | (key[None, :] == arg)
            s = np.matmul(qf, kk[:, :, key0: key0 + 64].transpose(0, 1, 3, 2))   # fp32 [B, H, T, 64]
            s = np.where(masked, np.float32(-np.inf), s)
            # the maxima are kept `shift` below the true ones (one fma): the probabilities are carried as 2^shift p
            mloc = (s.max(-1).astype(np.float64) * np.float64(c) - np.float64(shift)).astype(np.float32)
            m_new = np.maximum(m, mloc)
            m_use = np.where(m_new > -np.inf, m_new, np.float32(0))
            alpha = np.exp2((m - m_use).astype(np.float64)).astype(np.float32)
            # fma(s, c, -m_use): the product of two fp32 is exact in float64
            p = np.exp2(s.astype(np.float64) * np.float64(c) - m_use[..., None].astype(np.float64)).astype(np.float32)
            p = np.where(np.isnan(p), np.float32(0), p)
            vblk = vv[:, :, key0: key0 + 64]
            if name == "double_key" and key0 <= arg < key0 + 64:
                p = np.concatenate([p, p[..., arg - key0: arg - key0 + 1]], axis=-1)
                vblk = np.concatenate([vblk, vblk[:, :, arg - key0: arg - key0 + 1]], axis=2)
            if name == "swap_v" and key0 <= arg[0] < key0 + 64:
                a, b = arg[0] - key0, arg[1] - key0
                vblk = vblk.copy()
                vblk[:, :, [a, b]] = vblk[:, :, [b, a]]
            l_new = l * alpha + p.sum(-1, dtype=np.float32)
            o_new = o * alpha[..., None] + np.matmul(p.astype(np.float16).astype(np.float32), vblk)
            m, l, o = np.where(run, m_new, m), np.where(run, l_new, l), np.where(run[:, None], o_new, o)
        inv = np.where(l > 0, np.float32(1) / np.where(l > 0, l, np.float32(1)), np.float32(0))
        out = (o * inv[..., None]).astype(np.float16).transpose(0, 2, 1, 3).copy()
    if name == "swap_rows_32":
        src = np.where((t ^ 32) < T, t ^ 32, t)
        out = out[:, src]
    return out


def emu(mutant=None, shift=P_SHIFT):
    return lambda q, k, v, keys, koff, scale: emulate(q, k, v, keys, koff, scale, mutant, shift)


# ---- the table and the guard -------------------------------------------------------------------------------------------------

def test_coverage_guard_holds_for_every_table_row():
    edges.check_coverage()
    r = edges.reach(edges.ROWS[1][0])
    assert r["nblk"] == [2, 4, 5] and r["skip"] and r["interior"] and r["edge"]
    assert edges.reach(edges.ROWS[5][1])["nblk"] == [0, 2] and edges.reach(edges.ROWS[5][0])["nblk"] == [2, 3]
    assert edges.reach(edges.ROWS[2][0])["nblk"] == [3, 4]


def test_sweeps_visit_every_key_row():
    for row in (1, 2):
        s = edges.ROWS[row][0]
        heads = s.B * s.Hkv
        n = ac.sweep_launches(s.keys, heads)
        assert n == {1: 20, 2: 30}[row]
        seen = np.concatenate([ac.sweep(s.keys, heads, i) for i in range(n)])
        assert set(seen.tolist()) == set(range(s.keys))
        assert all(len(set(ac.sweep(s.keys, heads, i).tolist())) == heads for i in range(n))


def test_prefill_reference_against_a_plain_loop():
    """The vectorised reference against the definition written out per head and row: grouped heads, an offset, a cache longer
    than keys with NaN behind it, and queries with nothing to attend."""
    rng = np.random.default_rng(3)
    B, T, H, Hkv, keys, D = 2, 7, 4, 2, 9, 8
    q, k, v = ac.normal_f16(rng, (B, T, H, D)), ac.normal_f16(rng, (B, Hkv, keys + 3, D)), ac.normal_f16(rng, (B, Hkv, keys + 3, D))
    ac.poison_tail(k, keys), ac.poison_tail(v, keys)
    for koff in (2, 0, -3, 50):
        got, absmean = ac.prefill_reference(q, k, v, keys, koff, 0.4)
        assert not np.isnan(got).any()
        for b in range(B):
            for h in range(H):
                for t in range(T):
                    n = min(keys, max(0, t + koff + 1))
                    assert n == ac.prefill_counts(T, keys, koff)[t]
                    w = np.array([np.exp(0.4 * np.dot(q[b, t, h].astype(np.float64), k[b, h // 2, s].astype(np.float64))) for s in range(n)])
                    x = v[b, h // 2, :n].astype(np.float64)
                    want = (w[:, None] * x).sum(0) / w.sum() if n else np.zeros(D)
                    wabs = (w[:, None] * np.abs(x)).sum(0) / w.sum() if n else np.zeros(D)
                    assert np.allclose(got[b, t, h], want, rtol=1e-12, atol=1e-14) and np.allclose(absmean[b, t, h], wabs, rtol=1e-12, atol=1e-14)


# ---- the conditions the GPU assertions rest on --------------------------------------------------------------------------------

@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_staircase_gap_is_200(row, i, D):
    """The hot key beats EVERY random row of its head by >= 200 (so wherever it is placed), the hotter key beats the hot one by
    >= 200, V has no zeros, the queries are identical down a kv-head group and differ between kv heads."""
    s = edges.ROWS[row][i]
    c = edges.staircase_case(s, D)
    assert np.exp(np.float64(-ac.GAP_MIN)) < 2.0 ** -149 / 2
    assert ac.hot_gap(c["q1"], c["k"][:, :, : s.keys], c["hot"], c["scale"]) >= ac.GAP_MIN
    q64 = c["q1"].astype(np.float64)
    s_hot = (q64 * c["hot"].astype(np.float64)).sum(-1) * c["scale"]
    s_hotter = (q64 * c["hotter"].astype(np.float64)).sum(-1) * c["scale"]
    assert (s_hotter - s_hot).min() >= ac.GAP_MIN and np.isfinite(c["hotter"].astype(np.float64)).all()
    assert (c["v"][:, :, : s.keys] != 0).all()
    assert np.isnan(c["k"][:, :, s.keys:]).all() and np.isnan(c["v"][:, :, s.keys:]).all() and c["k"].shape[2] > s.keys
    g = s.H // s.Hkv
    assert (c["q"] == c["q"][:, :1]).all() and all((c["q"][:, :, h] == c["q"][:, :, (h // g) * g]).all() for h in range(s.H))
    if s.Hkv > 1:
        assert not (c["q1"][:, 0] == c["q1"][:, 1]).all()


PAIRED = [(r, i, D, kind) for r, i, D in TABLE for kind in ("diagonal", "permutation")
          if (r in (1, 2, 3, 4)) or (r == 6 and kind == "permutation")]


@pytest.mark.parametrize("row,i,D,kind", PAIRED, ids=["row%d.%d-D%d-%s" % p for p in PAIRED])
def test_pairing_gap_is_200(row, i, D, kind):
    """Every query's own hot score exceeds every other score it may attend -- the other queries' hot keys included -- by
    >= 200; pi is injective and within reach; the float64 reference rounds to V[pi(t)]."""
    s = edges.ROWS[row][i]
    c = edges.pairing_case(s, D, kind)
    koff = edges.koff_of(s)
    assert ac.pairing_gap(c["q0"], c["k"], c["pi"], s.keys, koff, c["scale"]) >= ac.GAP_MIN
    assert c["gap"] >= ac.GAP_MIN + ac.PAIR_MARGIN and np.isfinite(c["k"][:, :, : s.keys].astype(np.float64)).all()
    for b in range(s.B):
        for h in range(s.Hkv):
            pi = c["pi"][b, h]
            assert len(set(pi.tolist())) == s.T and (pi >= 0).all() and (pi <= np.minimum(s.keys - 1, np.arange(s.T) + koff)).all()
            if kind == "diagonal":
                assert (pi == np.arange(s.T) + koff).all()
    if kind == "permutation" and koff > 0 and s.T > 1:
        assert (c["pi"] != np.arange(s.T) + koff).any()
    ref, _ = ac.prefill_reference(c["q"], c["k"], c["v"], s.keys, koff, c["scale"])
    assert not ac.check_pairing(ref.astype(np.float16), c).any()
    assert (c["v"][:, :, : s.keys] != 0).all() and np.isnan(c["k"][:, :, s.keys:]).all() and np.isnan(c["v"][:, :, s.keys:]).all()


@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_census_sees_one_dropped_or_doubled_row(row, i, D):
    """Dropping or doubling ANY single attendable row moves some channel of that query row by more than 3 fp16 ulp, at
    every prefix length the shape has."""
    s = edges.ROWS[row][i]
    c = edges.census_case(s, D)
    a = np.abs(c["v"][:, :, : s.keys].astype(np.float64))
    assert a.min() >= 1 and a.max() == 8 and (a.max(-1) == 8).all() and (a == np.round(a)).all() and not c["q"].any()
    counts = ac.prefill_counts(s.T, s.keys, edges.koff_of(s))
    if not counts.any():
        return
    drop, dbl = ac.prefix_census_shift_ulps(c["v"], counts)
    assert drop > 3.0 and dbl > 3.0, (drop, dbl)


@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_ramp_block_maxima_rise(row, i, D):
    """For the last query row the float64 maxima of the 64-key blocks rise strictly from block to block: every block after the
    first rescales the accumulator with 0 < alpha < 1."""
    s = edges.ROWS[row][i]
    for scaling in ("default", "one"):
        c = edges.random_case(s, D, scaling, True)
        if ac.prefill_counts(s.T, s.keys, edges.koff_of(s))[-1] == 0:
            continue
        bm = ac.block_maxima(c["q"], c["k"], s.keys, edges.koff_of(s), c["scale"])
        assert (np.diff(bm, axis=-1) > 0).all(), (scaling, bm)
        assert np.isfinite(c["k"][:, :, : s.keys].astype(np.float64)).all()


# ---- the emulation passes every family ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_emulation_passes_the_exact_families_and_the_census(row, i, D):
    """Bit for bit on the staircase, the diagonal and the permutation; within 1 ulp on the census."""
    s = edges.ROWS[row][i]
    if row in (1, 2):
        edges.drive_staircase_sweep(emu(), s, D)
    if row in (3, 6):
        edges.drive_staircase_edges(emu(), s, D)
    if row in (1, 2, 3, 4):
        edges.drive_pairing(emu(), s, D, "diagonal")
    if row in (1, 2, 3, 4, 6):
        edges.drive_pairing(emu(), s, D, "permutation")
    ulp = edges.drive_census(emu(), s, D)
    print("prefill-cases emulation row %d.%d D=%d: census %.4f ulp" % (row, i, D, ulp))


@pytest.mark.parametrize("row,i,D", TABLE, ids=TABLE_IDS)
def test_emulation_stays_within_the_random_bound(row, i, D):
    s = edges.ROWS[row][i]
    ratios = [edges.drive_random(emu(), s, D, scaling, ramp) for scaling, ramp in edges.RANDOM_KINDS]
    print("prefill-cases emulation row %d.%d D=%d: random ratios %s" % (row, i, D, ["%.3f" % r for r in ratios]))


def test_unshifted_probabilities_miss_the_random_bound():
    """What these tests found in the kernel, kept as a ninth mutant.  With the probabilities handed to the value product as
    plain fp16 p <= 1 (shift 0), every p below 2^-14 is an fp16 subnormal: its rounding error is absolute, up to 2^-25, not
    the relative 2^-11 the random bound allows for.  Row 2 at D = 64, scaling 1 with the ramp has a query (b 1, t 112, h 3)
    whose softmax is peaked (l = 1.00016) on key 141, whose value in channel 49 is 1.0e-5; six keys with p in [2^-25, 2^-14]
    and values of order 1 lie behind it.  Their rounding errors add up to 1.03e-7 = 1.7 fp16 spacings of the answer 1.7e-5,
    1.21 times the bound, in this emulation and on the MI355X alike.  Carried as 2^12 p the same probabilities keep 11 bits
    down to 2^-26."""
    s, D = ROW2, 64
    c = edges.random_case(s, D, "one", True)
    bound = ac.random_bound(c["ref"], c["absmean"])
    out0 = emulate(c["q"], c["k"], c["v"], s.keys, s.koff, 1.0, shift=0.0)
    out12 = emulate(c["q"], c["k"], c["v"], s.keys, s.koff, 1.0)
    r0 = np.abs(out0.astype(np.float64) - c["ref"]) / bound
    r12 = np.abs(out12.astype(np.float64) - c["ref"]) / bound
    print("prefill-cases unshifted %.4f at %s, shifted %.4f" % (r0.max(), np.unravel_index(r0.argmax(), r0.shape), r12.max()))
    assert r0.max() > 1.0 and np.unravel_index(r0.argmax(), r0.shape) == (1, 112, 3, 49)
    assert r12.max() <= 1.0
    assert _fails(edges.drive_random, emu(shift=0.0), s, D, "one", True)


def test_emulation_passes_the_two_step_variants_on_row_2():
    """Row 7 is row 2's shape: its staircase edges and two-step variants, on the emulation."""
    for D in edges.DIMS:
        edges.drive_staircase_edges(emu(), edges.ROWS[7][0], D)


# ---- every mutant fails some family on some table row ----------------------------------------------------------------------------

def _fails(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


ROW1, ROW2, ROW3_65, ROW6 = edges.ROWS[1][0], edges.ROWS[2][0], edges.ROWS[3][2], edges.ROWS[6][0]

MUTANTS = {
    # name: (mutant, [(driver, shape, further arguments)]) -- every listed run must fail, at both head sizes
    "mask_lt": (("mask_lt", None), [(edges.drive_pairing, ROW1, ("diagonal",)), (edges.drive_census, ROW2, ()),
                                    (edges.drive_staircase_sweep, ROW1, ())]),
    "mask_plus_one": (("mask_plus_one", None), [(edges.drive_census, ROW1, ()), (edges.drive_staircase_sweep, ROW1, ()),
                                                (edges.drive_census, ROW2, ())]),
    "edge_from_last_row": (("edge_from_last_row", None), [(edges.drive_census, ROW1, ()), (edges.drive_census, ROW2, ()),
                                                          (edges.drive_staircase_sweep, ROW1, ())]),
    "drop_key": (("drop_key", 101), [(edges.drive_staircase_sweep, ROW1, ()), (edges.drive_census, ROW1, ()),
                                     (edges.drive_pairing, ROW2, ("permutation",)), (edges.drive_census, ROW6, ())]),
    "double_key": (("double_key", 101), [(edges.drive_census, ROW1, ()), (edges.drive_census, ROW2, ()), (edges.drive_census, ROW6, ())]),
    "swap_v": (("swap_v", (64, 68)), [(edges.drive_staircase_sweep, ROW1, ()), (edges.drive_pairing, ROW1, ("diagonal",)),
                                      (edges.drive_staircase_edges, ROW3_65, ()), (edges.drive_pairing, ROW2, ("permutation",))]),
    "swap_rows_32": (("swap_rows_32", None), [(edges.drive_pairing, ROW1, ("diagonal",)), (edges.drive_pairing, ROW2, ("permutation",)),
                                              (edges.drive_census, ROW3_65, ())]),
    "kv_head_modulo": (("kv_head_modulo", None), [(edges.drive_staircase_sweep, ROW2, ()), (edges.drive_pairing, ROW2, ("diagonal",)),
                                                  (edges.drive_census, ROW2, ()), (edges.drive_random, ROW2, ("default", False))]),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
@pytest.mark.parametrize("D", edges.DIMS)
def test_mutant_is_caught(name, D):
    mutant, runs = MUTANTS[name]
    for fn, s, extra in runs:
        assert _fails(fn, emu(mutant), s, D, *extra), "%s passes %s on %s at D = %d" % (name, fn.__name__, s, D)
