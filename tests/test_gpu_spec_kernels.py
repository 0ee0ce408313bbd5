"""The two kernels of speculative greedy decoding on the GPU (eetq_spec_ngram_draft_i64, eetq_spec_accept_f16) against the NumPy
restatements of their contracts (tests/spec_ref.py): exact integer equality, through both bindings.

Draft histories are built from pairwise distinct filler tokens (no n-gram of them ever repeats) with the patterns under test
planted at chosen columns, so each case has exactly the hits it names.  Accept logits are N(0, 1) noise with one entry per row
raised to 12 (its argmax, whatever the noise), so the row argmaxes g are chosen, not found; the draft is g with chosen entries
changed, which sets every row's number of confirmed tokens."""
import numpy as np
import pytest
import torch

import spec_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", params=["ext", "ctypes"])
def ops(request):
    if request.param == "ext":
        import eetq_amd.ops as o
        if o.BOUNDARY != "ext":
            pytest.skip("the compiled operator module is not in use")
        return o
    import eetq_amd.ops_ctypes as o
    return o


# ---------------------------------------------------------------------------------------------------------------- the draft

def _filler(B, cols, seed=0):
    """pairwise distinct tokens >= 1000, shuffled: no token repeats anywhere"""
    rng = np.random.default_rng(seed)
    return (1000 + rng.permutation(B * cols)).reshape(B, cols).astype(np.int64)


def _draft(ops, hist, position, N, k, pad=0):
    """one launch on a copy of `hist` (row stride cols + pad); asserts equality with the reference and that nothing else was
    written; returns the draft"""
    hist = np.asarray(hist, dtype=np.int64)
    B, cols = hist.shape
    big = torch.full((B, cols + pad), -5, dtype=torch.int64, device=DEV)
    big[:, :cols] = torch.from_numpy(hist).to(DEV)
    before = big.clone()
    pos = torch.tensor([position], dtype=torch.int64, device=DEV)
    wide = torch.full((B, k + 3), -9, dtype=torch.int64, device=DEV)
    ops.ngram_draft(big[:, :cols], pos, wide[:, :k], N)
    got = wide[:, :k].cpu().numpy()
    want = ref.ngram_draft_ref(hist, position, N, k)
    assert np.array_equal(got, want), (position, N, k, got.tolist(), want.tolist())
    assert torch.equal(big, before) and int(pos) == position and (wide[:, k:] == -9).all()
    return got


@pytest.mark.parametrize("L", [1, 2, 257, 4099])
def test_draft_lengths_on_repetitive_rows(ops, L):
    """a 3-letter alphabet: hits of every length everywhere, the longest and most recent one must be found among thousands"""
    rng = np.random.default_rng(L)
    for alphabet, N, k in ((3, 3, 5), (3, 8, 15), (40, 2, 4), (2, 1, 1)):
        hist = rng.integers(0, alphabet, (2, L + 7)).astype(np.int64)
        _draft(ops, hist, L - 1, N, k)


def test_draft_no_hit_and_unigram_only(ops):
    h = _filler(1, 300)
    assert _draft(ops, h, 299, 3, 4).tolist() == [[h[0, 299]] * 4]                   # nothing repeats: the pending token
    h[0, 120] = h[0, 299]                                                           # the tail token once before, other neighbours
    assert _draft(ops, h, 299, 3, 4).tolist() == [h[0, 121:125].tolist()]            # a hit at n = 1 only
    assert _draft(ops, h, 299, 1, 2).tolist() == [h[0, 121:123].tolist()]


def test_draft_prefers_the_longest_then_the_most_recent(ops):
    h = _filler(1, 600)
    tail = h[0, 597:600].copy()
    h[0, 100:103] = tail                 # an old trigram hit
    h[0, 500] = tail[2]                  # a newer unigram hit
    h[0, 550:552] = tail[1:]             # a newer bigram hit
    assert _draft(ops, h, 599, 3, 3).tolist() == [h[0, 103:106].tolist()]            # n = 3 wins although it is the oldest
    assert _draft(ops, h, 599, 2, 3).tolist() == [h[0, 552:555].tolist()]            # capped at bigrams: the bigram hit
    assert _draft(ops, h, 599, 1, 3).tolist() == [h[0, 552:555].tolist()]            # unigrams: column 551 is the most recent
    h[0, 300:303] = tail                 # a second trigram hit, more recent than the first
    assert _draft(ops, h, 599, 3, 3).tolist() == [h[0, 303:306].tolist()]
    assert _draft(ops, h, 599, 8, 3).tolist() == [h[0, 303:306].tolist()]            # longer n-grams have no hit


def test_draft_period_one_and_wrap_into_itself(ops):
    h = _filler(1, 64)
    h[0, 62] = h[0, 63] = 7                                                         # the hit ends at L - 2
    assert _draft(ops, h, 63, 3, 6).tolist() == [[7] * 6]
    h = _filler(1, 64)
    x = int(h[0, 57])
    h[0, 60:64] = [x, 3, 4, x]                                                      # x . . x 3 4 x: the most recent x is followed by 3 4 x
    assert _draft(ops, h, 63, 2, 15).tolist() == [[3, 4, x] * 5]                     # ... which runs off the end into the draft itself
    assert _draft(ops, np.array([[1, 2, 3, 1, 2]]), 4, 2, 5).tolist() == [[3, 1, 2, 3, 1]]
    assert _draft(ops, np.array([[1, 2, 3, 1, 2]]), 4, 2, 15).tolist() == [([3, 1, 2] * 5)]


def test_draft_ngram_at_column_zero(ops):
    h = _filler(1, 40)
    h[0, 0:3] = h[0, 37:40]                                                         # the only hit starts at column 0
    assert _draft(ops, h, 39, 3, 3).tolist() == [h[0, 3:6].tolist()]
    assert _draft(ops, h, 39, 8, 3).tolist() == [h[0, 3:6].tolist()]                 # n > e + 1 may not reach before column 0
    h2 = np.array([[4, 6, 0, 4, 6]])
    assert _draft(ops, h2, 4, 8, 3).tolist() == [[0, 4, 6]]


@pytest.mark.parametrize("e", [255, 256, 257, 1023, 1024, 4097])
def test_draft_hit_at_a_chosen_column(ops, e):
    """L = 4099 (four strides of the workgroup and a remainder): the single bigram hit ends at column e; 4097 = L - 2 is the last
    candidate"""
    L = 4099
    h = _filler(1, L + 20)
    if e == L - 2:                        # the hit overlaps the tail: ... a a a
        h[0, L - 3:L] = 77
        assert _draft(ops, h, L - 1, 2, 4).tolist() == [[77] * 4]
        return
    h[0, e - 1:e + 1] = h[0, L - 2:L]
    assert _draft(ops, h, L - 1, 2, 4).tolist() == [h[0, e + 1:e + 5].tolist()]
    assert _draft(ops, h, L - 1, 8, 4).tolist() == [h[0, e + 1:e + 5].tolist()]


def test_draft_rows_differ_stride_and_clamps(ops):
    cols = 90
    h = _filler(3, cols)
    h[1, 10:12] = h[1, 88:90]             # row 1: a bigram hit; row 0: none; row 2: period 1
    h[2, 88] = h[2, 89]
    got = _draft(ops, h, cols - 1, 3, 4, pad=13)                                    # a row stride larger than cols
    assert got.tolist() == [[h[0, 89]] * 4, h[1, 12:16].tolist(), [h[2, 89]] * 4]
    assert np.array_equal(_draft(ops, h, cols + 40, 3, 4, pad=2), got)              # L clamped at cols
    assert _draft(ops, h, -3, 3, 2).tolist() == [[h[b, 0]] * 2 for b in range(3)]    # ... and at 1
    # only the first position + 1 columns are tokens: row 1's hit is seen from position 89 only
    assert _draft(ops, h, 60, 3, 4).tolist() == [[h[b, 60]] * 4 for b in range(3)]


# --------------------------------------------------------------------------------------------------------------- the accept

def _steered(B, T, V, seed, pad=0):
    """(logits [B, T, V] fp16 on the device with position stride V + pad, their argmaxes g [B, T])"""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((B, T, V)).astype(np.float16)
    g = rng.integers(0, V, (B, T))
    g[0, 0], g[-1, -1] = 0, V - 1                                                    # the first and the last entry of a row too
    np.put_along_axis(lg, g[..., None], np.float16(12.0), axis=-1)
    dev = torch.zeros(B, T, V + pad, dtype=torch.float16, device=DEV)
    dev[:, :, :V] = torch.from_numpy(lg).to(DEV)
    return dev[:, :, :V], lg, g.astype(np.int64)


def _draft_confirming(g, a, V):
    """g[:, :k] with entry a[b] of row b changed (a[b] == k: none): row b confirms exactly a[b] tokens.  Entries behind the
    first wrong one stay right: only LEADING matches may count."""
    d = g[:, :-1].copy()
    for b, ab in enumerate(a):
        if ab < d.shape[1]:
            d[b, ab] = (d[b, ab] + 1) % V
    return d


def _accept(ops, lg_dev, lg, draft, column=1, position=20, limit=1000, out_cols=40, hist_cols=64, two_d_tok=True):
    """one launch on fresh state; asserts equality with the reference on every state tensor; returns adv"""
    B = lg.shape[0]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device=DEV)
    out0, hist0 = np.full((B, out_cols), -7), np.full((B, hist_cols), -3)
    tok0, stats0 = np.full((B, 1) if two_d_tok else (B,), -1), np.array([5, 11])
    out, hist, tok, stats, d = t(out0), t(hist0), t(tok0), t(stats0), t(draft)
    col, pos, lim = t([[column]]), t([position]), t([limit])
    ops.spec_accept(lg_dev, d, out, col, tok, pos, lim, hist, stats)
    w_out, w_col, w_tok, w_pos, w_hist, w_stats, adv = ref.spec_accept_ref(lg, draft, out0, column, tok0, position, limit, hist0, stats0)
    assert int(col) == w_col and int(pos) == w_pos and int(lim) == limit, (int(col), w_col, int(pos), w_pos)
    assert np.array_equal(out.cpu().numpy(), w_out) and np.array_equal(hist.cpu().numpy(), w_hist)
    assert np.array_equal(tok.cpu().numpy(), w_tok) and stats.tolist() == w_stats.tolist()
    assert np.array_equal(d.cpu().numpy(), draft)
    return adv


@pytest.mark.parametrize("V", [512, 32003])
@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("B", [1, 3])
def test_accept_every_count_and_the_row_minimum(ops, V, k, B):
    """every n in 0 .. k as the minimum over rows, held by each row in turn while the others confirm more; a position stride
    larger than V (odd V + an odd pad: rows on 2-byte boundaries)"""
    lg_dev, lg, g = _steered(B, k + 1, V, seed=V + 16 * k + B, pad=5)
    assert lg_dev.stride(1) == V + 5
    rng = np.random.default_rng(k)
    for n in range(k + 1):
        a = [int(rng.integers(n, k + 1)) for _ in range(B)]
        a[n % B] = n
        assert _accept(ops, lg_dev, lg, _draft_confirming(g, a, V)) == n + 1


def test_accept_argmax_rule(ops):
    """first index on ties, a NaN is the maximum (the first NaN), -0 == +0, an all -inf row; the drafts are the reference's
    tokens, so every position is reached"""
    V, k = 512, 4
    lg = np.random.default_rng(1).standard_normal((1, k + 1, V)).astype(np.float16)
    lg[0, 0, [300, 17, 450]] = 9.0                     # a tie: 17
    lg[0, 1, 200] = 30.0
    lg[0, 1, [401, 77]] = np.nan                       # NaN beats 30: 77
    lg[0, 2, :] = -0.0
    lg[0, 2, 5] = 0.0                                  # -0 == +0: index 0
    lg[0, 3, :] = -np.inf                              # index 0
    lg[0, 4, V - 1] = np.inf
    want = [17, 77, 0, 0, V - 1]
    assert [ref.greedy_token(lg[0, t]) for t in range(k + 1)] == want
    assert torch.from_numpy(lg[0].astype(np.float32)).argmax(-1).tolist() == want      # torch.argmax agrees with the reference
    dev = torch.from_numpy(lg).to(DEV)
    assert _accept(ops, dev, lg, np.array([want[:k]])) == k + 1
    assert _accept(ops, dev, lg, np.array([[17, 77, 5, 0]])) == 3                       # the +0 at index 5 is not the first zero


def test_accept_limit_and_ranges(ops):
    V, k, B = 512, 4, 3
    lg_dev, lg, g = _steered(B, k + 1, V, seed=3)
    n = 2
    d = _draft_confirming(g, [n, 4, 3], V)
    for room, adv in ((0, 0), (1, 1), (n, n), (n + 1, n + 1), (10 ** 12, n + 1), (-5, 0)):
        assert _accept(ops, lg_dev, lg, d, column=6, limit=6 + room) == adv
    full = _draft_confirming(g, [k, k, k], V)
    for room, adv in ((k, k), (k + 1, k + 1), (k + 2, k + 1)):
        assert _accept(ops, lg_dev, lg, full, column=0, limit=room) == adv
    # the output columns run off out_tokens, the history columns off hist; a negative column: skipped, the counters still move
    assert _accept(ops, lg_dev, lg, full, column=38, out_cols=40) == k + 1
    assert _accept(ops, lg_dev, lg, full, column=40, out_cols=40) == k + 1
    assert _accept(ops, lg_dev, lg, full, column=-2, limit=50) == k + 1
    assert _accept(ops, lg_dev, lg, full, position=60, hist_cols=64) == k + 1
    assert _accept(ops, lg_dev, lg, full, position=63, hist_cols=64) == k + 1
    assert _accept(ops, lg_dev, lg, full, two_d_tok=False) == k + 1


def test_accept_nothing_to_hand_over_leaves_the_state(ops):
    """adv = 0: every state tensor is byte-identical before and after, except stats[0]"""
    V, k, B = 512, 4, 2
    lg_dev, lg, g = _steered(B, k + 1, V, seed=4)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device=DEV)
    state = dict(draft=t(g[:, :k]), out=t(np.arange(B * 9).reshape(B, 9)), col=t([[7]]), tok=t([[41], [42]]), pos=t([30]), lim=t([7]),
                 hist=t(np.arange(B * 50).reshape(B, 50)), stats=t([3, 8]))
    before = {key: v.clone() for key, v in state.items()}
    logits_before = lg_dev.clone()
    s = state
    ops.spec_accept(lg_dev, s["draft"], s["out"], s["col"], s["tok"], s["pos"], s["lim"], s["hist"], s["stats"])
    assert s["stats"].tolist() == [4, 8]
    s["stats"][0] = 3
    for key in state:
        assert torch.equal(state[key], before[key]), key
    assert torch.equal(lg_dev, logits_before)


@pytest.mark.parametrize("V", [512, 32003])
def test_accept_with_every_draft_wrong_is_greedy_handover(ops, V):
    import eetq_amd.ops as base
    k, B = 4, 3
    lg_dev, lg, g = _steered(B, k + 1, V, seed=V, pad=5)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device=DEV)
    out_a, col_a, tok_a, pos_a = t(np.full((B, 12), -7)), t([[4]]), t(np.full((B, 1), -1)), t([9])
    out_b, col_b, tok_b, pos_b = out_a.clone(), col_a.clone(), tok_a.clone(), pos_a.clone()
    hist, stats = t(np.full((B, 30), -3)), t([0, 0])
    ops.spec_accept(lg_dev, t(_draft_confirming(g, [0] * B, V)), out_a, col_a, tok_a, pos_a, t([100]), hist, stats)
    first = lg_dev[:, 0]
    assert first.stride(0) == (k + 1) * (V + 5)
    base.greedy_handover(first, out_b, col_b, tok_b, pos_b)
    assert torch.equal(out_a, out_b) and torch.equal(col_a, col_b) and torch.equal(tok_a, tok_b) and torch.equal(pos_a, pos_b)
    assert int(col_a) == 5 and int(pos_a) == 10 and stats.tolist() == [1, 1] and hist[:, 10].tolist() == g[:, 0].tolist()


def test_both_launches_in_a_captured_graph():
    """draft -> accept on static tensors, captured once and replayed: the replays advance the device state as eager calls do"""
    import eetq_amd.ops as ops
    V, k, B, cols = 512, 4, 2, 48
    rng = np.random.default_rng(9)
    period = rng.permutation(V)[:6].astype(np.int64)            # the "model": token i of the period is followed by token i + 1
    nxt = {int(period[i]): int(period[(i + 1) % 6]) for i in range(6)}
    seq = [int(period[i % 6]) for i in range(9)]                # 9 tokens of the cycle: the last is pending
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int64, device=DEV)
    hist = torch.zeros(B, cols, dtype=torch.int64, device=DEV)
    hist[:, :9] = t(seq)
    pos, col, lim, stats = t([8]), t([[0]]), t([17]), t([0, 0])
    tok, out, draft = t([[seq[-1]]] * B), torch.full((B, 20), -1, dtype=torch.int64, device=DEV), torch.zeros(B, k, dtype=torch.int64, device=DEV)
    table = torch.zeros(V, dtype=torch.int64, device=DEV)
    for a, b in nxt.items():
        table[a] = b
    logits = torch.zeros(B, k + 1, V, dtype=torch.float16, device=DEV)

    def step():
        ops.ngram_draft(hist, pos, draft, 3)
        ids = torch.cat([tok, draft], dim=1)                                      # the verify rows
        logits.zero_()
        logits.scatter_(2, table[ids].unsqueeze(-1), 5.0)                         # the model's answer to every row
        ops.spec_accept(logits, draft, out, col, tok, pos, lim, hist, stats)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    assert int(col) == 5 and stats.tolist() == [1, 5]                             # the lookup was right: k + 1 tokens
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(4):
        graph.replay()
    want = [int(period[(9 + i) % 6]) for i in range(17)]
    assert int(col) == 17 and int(pos) == 25 and stats.tolist() == [5, 17]        # 5 + 5 + 5 + 2 (the limit), then nothing
    assert out[:, :17].tolist() == [want] * B and (out[:, 17:] == -1).all()
    assert hist[:, 9:26].tolist() == [want] * B and tok[:, 0].tolist() == [want[-1]] * B
