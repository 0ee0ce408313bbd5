"""The inputs of tests/test_gpu_attn_decode_edges.py meet the conditions its assertions rest on (tests/attn_cases.py): the
hot row's 200-unit gap, the census's sensitivity to one dropped or doubled row, the aperiodic mask, the float64 reference
itself -- and the table of shapes reaches the kernel paths it claims.  No GPU."""
import numpy as np
import pytest

import attn_cases as ac
import test_gpu_attn_decode_edges as edges

SHAPES = sorted({(D, S) for cases in edges.ROWS.values() for D, S, _ in cases})
CENSUS = sorted({(D, S) for r in (1, 2, 5, 7) for D, S, _ in edges.ROWS[r]})


def test_coverage_guard_holds_for_every_table_row():
    edges.check_coverage()
    assert edges.merge_jn(128, 130) == [8, 8, 1] and edges.merge_jn(64, 33) == [3] and edges.merge_jn(64, 65) == [4, 1]
    assert edges.long_trips(128, 700, 0, 2) == [4, 2] and edges.long_trips(128, 700, 1, 2) == [4, 2]
    assert edges.long_trips(128, 256, 0, 1) == [] and edges.long_trips(128, 257, 0, 1) == [1]
    assert edges.long_trips(64, 513, 0, 1) == [1] and edges.long_trips(64, 1500, 0, 2) == [4, 4]


def test_sweep_visits_every_position_once_per_head_slot():
    for n, heads in ((700, 64), (1040, 64), (17, 64), (1, 64), (96, 64)):
        seen = np.concatenate([ac.sweep(n, heads, i) for i in range(ac.sweep_launches(n, heads))])
        assert set(seen.tolist()) == set(range(n))
        if n >= heads:
            assert all(len(set(ac.sweep(n, heads, i).tolist())) == heads for i in range(ac.sweep_launches(n, heads)))


@pytest.mark.parametrize("D,S", SHAPES)
def test_hot_row_gap_is_200(D, S):
    """From the float64 scores: the hot key beats EVERY row of the random cache by >= 200 (so wherever it is placed), the
    hotter key of the variants beats the hot one by >= 200, and exp(-200) is 0 in fp32."""
    assert np.exp(np.float64(-ac.GAP_MIN)) < 2.0 ** -149 / 2   # rounds to 0 even with fp32 denormals
    for B, H in ((edges.HOT_B, edges.HOT_H), (edges.VAR_B, edges.VAR_H)):
        c = ac.hot_base(B, H, S, D, seed=1000 * D + S)
        assert ac.hot_gap(c["q"], c["k"], c["hot"], c["scale"]) >= ac.GAP_MIN
        q64 = c["q"].astype(np.float64)
        s_hot = (q64 * c["hot"].astype(np.float64)).sum(-1) * c["scale"]
        s_hotter = (q64 * c["hotter"].astype(np.float64)).sum(-1) * c["scale"]
        assert (s_hotter - s_hot).min() >= ac.GAP_MIN and np.isfinite(c["hotter"].astype(np.float64)).all()
        assert (c["v"] != 0).all()
        # the reference agrees: with the hot key at row r the float64 answer rounds to V[r]
        r = ac.sweep(S, B * H, 3).reshape(B, H)
        k = c["k"].copy()
        ib, ih = np.meshgrid(np.arange(B), np.arange(H), indexing="ij")
        k[ib, ih, r] = c["hot"]
        ref = ac.reference(c["q"], k, c["v"], S, c["scale"]).astype(np.float16)
        assert np.array_equal(ref.view(np.int16), c["v"][ib, ih, r].view(np.int16))


@pytest.mark.parametrize("D,S,splits", edges.ONE_LAUNCH)
def test_new_token_gap_is_200(D, S, splits):
    """The same gap for the one-launch form's new token, after the fp16 rotation of q and of the hot key."""
    assert ac.new_token_gap(ac.new_token_hot(2, 16, S, D, seed=S + D + splits)) >= ac.GAP_MIN


def test_mask_driven_gap_is_200():
    assert float(np.float16(-200.0)) == -200.0   # finite and exact in fp16: K = 0 leaves the mask as the only score


@pytest.mark.parametrize("D,S", CENSUS)
def test_census_sees_one_dropped_or_doubled_row(D, S):
    """Dropping or doubling ANY single row moves some channel of the float64 answer by more than 3 fp16 ulp -- three times
    the bound the GPU test asserts -- at every valid length the GPU test uses."""
    v, _ = ac.census_values(edges.CEN_B, edges.CEN_HKV, S, D, seed=D + S)
    a = np.abs(v.astype(np.float64))
    assert a.min() >= 1 and a.max() == 8 and (a.max(-1) == 8).all() and (a == np.round(a)).all()
    for sv in ([s for s in edges.SV_SWEEP if s] if (D, S, 2) in edges.ROWS[7] else [S]):
        drop, dbl = ac.census_shift_ulps(v, sv)
        assert drop > 3.0, (sv, drop)
        assert sv == 1 or dbl > 3.0, (sv, dbl)   # sv == 1: 2v / 2 == v, invisible to any softmax


def test_fp16_ulp():
    x = np.array([0.0, 2.0 ** -24, 2.0 ** -14, 0.75, 1.0, 1.5, 2.0, -3.0, 2047.0])
    want = np.array([2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 1.0])
    assert np.array_equal(ac.fp16_ulp(x), want)
    for val in (0.3, 1.0, 5.5, 1000.0):
        h = np.float16(val)
        assert float(np.nextafter(h, np.float16(np.inf))) - float(h) == ac.fp16_ulp(float(h))


def test_random_mask_is_mixed_and_aperiodic():
    for width in (96 + 24, 700 + 24, 1500 + 24):
        m = ac.random_mask(2, width, seed=width).astype(np.float64)
        hole, zero = np.isneginf(m), m == 0
        finite = ~hole & ~zero
        assert 0.1 < hole.mean() < 0.2 and 0.2 < zero.mean() < 0.4 and finite.mean() > 0.4
        assert (m[finite] < 0).all() and np.isfinite(m[finite]).all()
        for period in (16, 32, 64):          # no pattern of the block sizes or their multiples
            assert not np.array_equal(hole[:, period:], hole[:, :-period])
            assert not np.array_equal(zero[:, period:], zero[:, :-period])


def test_reference_against_a_plain_loop():
    """The vectorised reference against the definition written out per head and row: grouped heads, a mask wider than the
    cache, a valid length, a fully masked query, sv = 0."""
    rng = np.random.default_rng(11)
    B, H, Hkv, S, D, sv = 2, 4, 2, 13, 8, 9
    q, k, v = ac.normal_f16(rng, (B, H, D)), ac.normal_f16(rng, (B, Hkv, S, D)), ac.normal_f16(rng, (B, Hkv, S, D))
    mask = ac.random_mask(B, S + 5, seed=3)
    mask[1, :sv] = -np.inf
    got = ac.reference(q, k, v, sv, 0.4, mask)
    for b in range(B):
        for h in range(H):
            w = np.array([np.exp(0.4 * np.dot(q[b, h].astype(np.float64), k[b, h // 2, s].astype(np.float64))
                                 + float(mask[b, s])) for s in range(sv)])
            want = (w[:, None] * v[b, h // 2, :sv].astype(np.float64)).sum(0) / w.sum() if w.sum() > 0 else np.zeros(D)
            assert np.allclose(got[b, h], want, rtol=1e-12, atol=1e-14)
    assert not got[1].any() and got[0].any()
    assert not ac.reference(q, k, v, 0, 0.4, mask).any()


def test_rotation_keeps_the_pairing():
    """rope_neox_f16 at position 0 is the identity; elsewhere it preserves q . k to fp16 accuracy."""
    rng = np.random.default_rng(5)
    x = ac.normal_f16(rng, (2, 3, 64))
    table = ac.rope_table(64, 128)
    assert np.array_equal(ac.rope_neox_f16(x, table, np.array([0, 0])), x)
    y = ac.rope_neox_f16(x, table, np.array([17, 101])).astype(np.float64)
    assert np.allclose((y * y).sum(-1), (x.astype(np.float64) ** 2).sum(-1), rtol=5e-3)
