"""Sampling decode hand-over on the GPU (eetq_sample_handover_f16): every case feeds explicit random numbers and demands the
EXACT token of the float64 reference (tests/sampling_ref.py).  The numbers sit at the midpoints of reference intervals wider
than 2^-11 and every top_p is at least 2^-12 from every class boundary (both asserted on the reference), so the kernel's fp32
exponentials (error ~2^-18) cannot change the answer.

Rows of V >= 1001 are N(0, 1) with a head of 12 distinct logits in [24, 25): the head carries > 99 % of the mass at every
temperature used, so the cuts of top_p = 0.05 / 0.5 / 0.9 / 0.95 fall inside head intervals (a fp16 bulk of 10^5 entries has
class boundaries every ~10^-4 and no gap of 2^-11 anywhere), while the k-th value of top-k 50 lies in the tie-rich bulk.
The targets of a setting are the first and the last survivor whose interval is wider than 2^-11 and three in between."""
import numpy as np
import pytest
import torch

import sampling_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE, MARGIN = 2.0 ** -11, 2.0 ** -12


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


def _rows(V, B, seed):
    rng = np.random.default_rng(seed)
    if V < 1001:
        return (rng.standard_normal((B, V)) * 2).astype(np.float16)
    lg = rng.standard_normal((B, V)).astype(np.float16)
    for b in range(B):
        lg[b, rng.choice(V, 12, replace=False)] = (24 + rng.choice(64, 12, replace=False) / 64.0).astype(np.float16)
    return lg


def _state(B, col=2, cols=6):
    return (torch.full((B, cols), -7, dtype=torch.int64, device=DEV), torch.tensor([[col]], dtype=torch.int64, device=DEV),
            torch.full((B, 1), -1, dtype=torch.int64, device=DEV), torch.tensor([40], dtype=torch.int64, device=DEV))


def _draw(ops, lg, params, u=None, done=None, col=2):
    """one call on fresh counters; checks the bookkeeping; returns the tokens"""
    B = lg.shape[0]
    out, c, tok, pos = _state(B, col)
    ops.sample_handover(lg, out, c, tok, pos, params, done,
                        None if u is None else torch.tensor(np.asarray(u, dtype=np.float32), device=DEV))
    assert int(c) == col + 1 and int(pos) == 41
    if 0 <= col < out.shape[1]:
        assert torch.equal(out[:, col], tok[:, 0])
        out[:, col] = -7
    assert (out == -7).all()
    return tok[:, 0].cpu().numpy()


def _targets(r):
    """(token, u) pairs of one reference row: u at the midpoint of intervals wider than 2^-11"""
    if r.special is not None:
        return [(r.fixed, 0.5)] * 5
    wide = np.nonzero(r.hi - r.lo > WIDE)[0]
    assert wide.size >= 1
    pick = wide[np.unique(np.linspace(0, wide.size - 1, 5).round().astype(int))]
    res = []
    for i in pick:
        u = np.float32((r.lo[i] + r.hi[i]) / 2)
        assert u - r.lo[i] >= MARGIN and r.hi[i] - u >= MARGIN
        res.append((int(r.order[i]), u))
    return res


FILTERS = [(0, 1.0), (1, 1.0), (2, 1.0), (50, 1.0), ("V", 1.0), ("V+5", 1.0), (0, 0.05), (0, 0.5), (0, 0.95), (50, 0.9)]


@pytest.mark.parametrize("V,B", [(1, 1), (7, 2), (1001, 3), (32000, 4), (128256, 1)])
def test_exact_tokens(ops, V, B):
    host = _rows(V, B, seed=V + B)
    dev = torch.from_numpy(host).to(DEV)
    cases = [(host, dev)]
    if V == 1001:
        cases.append((host[:, 1:], dev[:, 1:]))            # rows that are not 16-byte aligned
    for h, d in cases:
        Vv = h.shape[1]
        for T in (0.5, 1.0, 1.7):
            for k, p in FILTERS:
                k = Vv if k == "V" else Vv + 5 if k == "V+5" else k
                rows = [ref.sample_row(h[b], T, top_k=k, top_p=p) for b in range(B)]
                for r in rows:
                    assert r.p_margin >= MARGIN, (Vv, T, k, p, r.p_margin)
                tg = [_targets(r) for r in rows]
                if Vv >= 1000 and (k == 0 or k >= 50) and p >= 0.9:
                    assert all(len(t) == 5 for t in tg)
                params = ops.sampling_params(temperature=T, top_k=k, top_p=p, device=DEV)
                for j in range(max(len(t) for t in tg)):
                    want = [t[j % len(t)][0] for t in tg]
                    got = _draw(ops, d, params, u=[t[j % len(t)][1] for t in tg])
                    assert got.tolist() == want, (Vv, T, k, p, j)


def test_ties(ops):
    row = np.full(1001, -30.0, dtype=np.float16)
    row[[10, 700, 20, 500]] = [5.0, 4.0, 4.0, 3.0]
    dev = torch.from_numpy(row)[None].to(DEV)
    # the 2nd and 3rd values are equal: top-k 2 keeps both; a tie straddling the p cut (0.53 < 0.6 < 0.53 + 0.2) stays whole
    for kw in (dict(top_k=2), dict(top_p=0.6)):
        r = ref.sample_row(row, 1.0, **kw)
        assert r.order.tolist() == [10, 20, 700] and r.p_margin >= MARGIN
        params = ops.sampling_params(temperature=1.0, device=DEV, **kw)
        for i in range(3):                                 # i = 2: the highest-index member of the tie
            assert r.hi[i] - r.lo[i] > WIDE
            assert _draw(ops, dev, params, u=[(r.lo[i] + r.hi[i]) / 2]).tolist() == [r.order[i]]
    flat = torch.full((1, 128256), 1.5, dtype=torch.float16, device=DEV)    # one class of 128 256: uniform
    params = ops.sampling_params(temperature=0.9, device=DEV)
    assert _draw(ops, flat, params, u=[0.5]).tolist() == [64128]
    assert _draw(ops, flat, params, u=[1.0 - 2.0 ** -24]).tolist() == [128255]
    assert _draw(ops, flat, params, u=[0.0]).tolist() == [0]


def test_non_finite_inputs(ops):
    inf, nan = np.inf, np.nan
    row = np.array([-inf, 1.0, nan, 2.0, -inf, 0.5, nan], dtype=np.float16)
    dev = torch.from_numpy(row)[None].to(DEV)
    r = ref.sample_row(row, 1.0)
    assert r.order.tolist() == [3, 1, 5]                   # -inf and NaN are never drawn
    params = ops.sampling_params(temperature=1.0, device=DEV)
    for i in range(3):
        assert _draw(ops, dev, params, u=[(r.lo[i] + r.hi[i]) / 2]).tolist() == [r.order[i]]
    assert _draw(ops, dev, params, u=[1.0 - 2.0 ** -24]).tolist() == [5]
    big = _rows(1001, 4, seed=9)
    big[0, [700, 33]] = inf                                # +inf: its first index, whatever u
    big[1] = -inf                                          # nothing above -inf: index 0
    big[2] = nan
    big[3, :900] = nan                                     # NaN next to finite entries: as -inf
    want3 = ref.sample_row(big[3], 1.0)
    assert want3.order.min() >= 900
    t3 = _targets(want3)
    for j in range(len(t3)):
        got = _draw(ops, torch.from_numpy(big).to(DEV), params, u=[0.3, 0.9, 0.5, t3[j][1]])
        assert got.tolist() == [33, 0, 0, t3[j][0]]


def test_temperature_zero_is_greedy_handover(ops):
    torch.manual_seed(5)
    for B, V in ((1, 32000), (4, 32000), (3, 1001), (2, 7), (1, 128256)):
        lg = (torch.randn(B, V, device=DEV) * 3).half()
        if V > 100:
            lg[0, 17] = lg[0, 90] = lg[0].max() + 1
            if B > 1:
                lg[1, 5] = float("nan")
                lg[1, 3] = float("inf")
            if B > 2:
                lg[2] = float("-inf")
        else:
            lg[0] = 0.0
            lg[0, 2] = -0.0
        for T in (0.0, -1.0, float("nan")):                # negative and NaN temperatures select greedy too
            params = ops.sampling_params(temperature=T, top_k=5, top_p=0.5, device=DEV)
            for view in (lg, lg[:, 1:]):
                for col in (2, 6, -1):                     # 6 and -1: outside the buffer, nothing written, still handed on
                    a, b = _state(B, col), _state(B, col)
                    ops.greedy_handover(view, *a)
                    ops.sample_handover(view, *b, params)
                    for x, y in zip(a, b):
                        assert torch.equal(x, y)
                    assert torch.equal(a[2][:, 0], view.argmax(-1)) and int(a[1]) == col + 1 and int(a[3]) == 41
                    if col == 2:
                        assert torch.equal(b[0][:, 2], view.argmax(-1)) and (b[0][:, [0, 1, 3, 4, 5]] == -7).all()
                    else:
                        assert (b[0] == -7).all()
    with pytest.raises(RuntimeError):
        ops.sample_handover(lg.float(), *_state(B), params)
    with pytest.raises(RuntimeError):
        ops.sample_handover(lg, *_state(B), params.long())


def test_own_random_numbers_are_philox(ops):
    flat = torch.zeros(4, 1001, dtype=torch.float16, device=DEV)
    for seed in (0, 2 ** 63 + 5):
        params = ops.sampling_params(temperature=1.0, seed=seed, device=DEV)
        for col in (0, 1, 2 ** 32 + 3):
            u = [ref.philox_uniform(seed, col, b) for b in range(4)]
            own = _draw(ops, flat, params, col=col)
            assert own.tolist() == _draw(ops, flat, params, u=u, col=col).tolist()
            assert own.tolist() == [int(np.float64(x) * 1001) for x in u]       # a flat row: token = floor(1001 u)
    flat = torch.zeros(64, 1001, dtype=torch.float16, device=DEV)
    base = _draw(ops, flat, ops.sampling_params(seed=1, device=DEV), col=3)
    assert len(set(base.tolist())) > 32
    assert (base != _draw(ops, flat, ops.sampling_params(seed=2, device=DEV), col=3)).any()
    assert (base != _draw(ops, flat, ops.sampling_params(seed=1, device=DEV), col=4)).any()
    assert (base == _draw(ops, flat, ops.sampling_params(seed=1, device=DEV), col=3)).all()


def test_eos_and_done(ops):
    lg = torch.from_numpy(_rows(1001, 3, seed=4)).to(DEV)
    g = lg.argmax(-1).tolist()
    params = ops.sampling_params(temperature=0.0, eos_token_id=g[1], pad_token_id=77, device=DEV)
    done = torch.zeros(3, dtype=torch.int32, device=DEV)
    assert _draw(ops, lg, params, done=done).tolist() == g and done.tolist() == [0, 1, 0]
    lg[1] = float("nan")                                   # a finished row is not looked at
    assert _draw(ops, lg, params, done=done).tolist() == [g[0], 77, g[2]] and done.tolist() == [0, 1, 0]
    sampled = ops.sampling_params(temperature=1.0, eos_token_id=g[1], pad_token_id=77, device=DEV)
    assert _draw(ops, lg, sampled, u=[0.5] * 3, done=done)[1] == 77
    # a SAMPLED draw of the EOS token sets the flag too: row 2 is aimed at its last wide survivor, made the EOS token
    eos2, u2 = _targets(ref.sample_row(lg[2].cpu().numpy(), 1.0))[-1]
    assert eos2 != g[2]
    aimed = ops.sampling_params(temperature=1.0, eos_token_id=eos2, pad_token_id=77, device=DEV)
    assert _draw(ops, lg, aimed, u=[0.0, 0.0, u2], done=done).tolist() == [g[0], 77, eos2] and done.tolist() == [0, 1, 1]
    assert _draw(ops, lg, aimed, u=[0.0, 0.0, u2], done=done).tolist() == [g[0], 77, 77]
    done[2] = 0
    lg[1] = lg[0]
    nodone = _draw(ops, lg, ops.sampling_params(temperature=0.0, eos_token_id=g[0], pad_token_id=77, device=DEV))
    assert nodone.tolist() == [g[0], g[0], g[2]]           # done=None: no EOS handling


def test_three_steps_under_graph_replay(ops):
    B, V = 2, 1001
    lg = torch.from_numpy(_rows(V, B, seed=6)).to(DEV)
    params = ops.sampling_params(temperature=1.0, seed=3, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    out, col, tok, pos = _state(B, col=0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sample_handover(lg, out, col, tok, pos, params, done)      # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(3):
                ops.sample_handover(lg, out, col, tok, pos, params, done)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    new = torch.from_numpy(_rows(V, B, seed=7)).to(DEV)
    eos = int(new[1].argmax())
    for T, e in ((1.3, None), (0.0, eos)):                 # rewritten logits, parameters and flags: no recapture
        lg.copy_(new)
        ops.sampling_params(temperature=T, top_k=40, seed=11, eos_token_id=e, pad_token_id=5, out=params)
        done.zero_()
        out.fill_(-7); col.fill_(1); pos.fill_(9)
        graph.replay()
        torch.cuda.synchronize()
        e_done = torch.zeros(B, dtype=torch.int32, device=DEV)
        e_out, e_col, e_tok, e_pos = _state(B, col=1)
        e_pos.fill_(9)
        for _ in range(3):
            ops.sample_handover(new, e_out, e_col, e_tok, e_pos, params, e_done)
        assert torch.equal(out, e_out) and torch.equal(tok, e_tok) and torch.equal(done, e_done)
        assert int(col) == int(e_col) == 4 and int(pos) == int(e_pos) == 12
        if e is not None:
            assert out[1, 1:4].tolist() == [eos, 5, 5] and done.tolist() == [0, 1]


@pytest.fixture(scope="module")
def tiny_llama():
    transformers = pytest.importorskip("transformers")
    from eetq_amd.utils import eet_accelerator
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=4, vocab_size=1001, max_position_embeddings=256)
    torch.manual_seed(0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device(DEV):
            model = transformers.LlamaForCausalLM(cfg)
    finally:
        torch.set_default_dtype(old)
    return eet_accelerator(model.eval(), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)


def test_graph_decoder_sampling(tiny_llama):
    from eetq_amd.utils import GraphDecoder
    B, P, NEW = 2, 9, 20
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, 1001, (B, P), generator=g).to(DEV)
    with torch.no_grad():
        plain = GraphDecoder(tiny_llama, B, P + NEW + 8)
        dec = GraphDecoder(tiny_llama, B, P + NEW + 8, sampling=True)
        want = plain.generate(prompt, NEW)
        assert torch.equal(dec.generate(prompt, NEW), want)                # do_sample=False: token for token
        assert dec.done.tolist() == [0, 0]
        eos = int(want[0, P + 6])                                          # a token row 0 is known to emit
        first = [int((want[b, P:] == eos).nonzero()[0]) if (want[b, P:] == eos).any() else NEW for b in range(B)]
        got = dec.generate(prompt, NEW, eos_token_id=eos, pad_token_id=3)
        for b in range(B):
            n = first[b]
            assert torch.equal(got[b, :P + min(n + 1, NEW)], want[b, :P + min(n + 1, NEW)])
            assert (got[b, P + n + 1:] == 3).all()
        assert dec.done.tolist() == [int(n < NEW) for n in first] and dec.done[0] == 1
        a = dec.generate(prompt, NEW, do_sample=True, temperature=1.5, seed=7)
        assert torch.equal(a, dec.generate(prompt, NEW, do_sample=True, temperature=1.5, seed=7))
        assert not torch.equal(a, dec.generate(prompt, NEW, do_sample=True, temperature=1.5, seed=8))
        assert a.shape == (B, P + NEW) and int(a.max()) < 1001 and int(a.min()) >= 0
        for kw in (dict(do_sample=True), dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(seed=1),
                   dict(eos_token_id=2), dict(pad_token_id=0)):
            with pytest.raises(ValueError, match="sampling=True"):
                plain.generate(prompt, NEW, **kw)
        assert torch.equal(plain.generate(prompt, NEW), want)


def test_negative_position_still_advances(ops):
    """The rows are counted in the upper bits of *position during a launch: a negative position (the greedy kernel takes one)
    must come out as position + 1 with the column advanced, at several rows."""
    lg = torch.from_numpy(_rows(1001, 4, seed=12)).to(DEV)
    params = ops.sampling_params(temperature=1.0, seed=5, device=DEV)
    for start in (-3, -1, 0, 2 ** 39 - 2, -2 ** 39):
        out, col, tok, pos = _state(4)
        pos.fill_(start)
        ops.sample_handover(lg, out, col, tok, pos, params)
        assert int(pos) == start + 1 and int(col) == 3 and torch.equal(out[:, 2], tok[:, 0]) and int(tok.min()) >= 0
