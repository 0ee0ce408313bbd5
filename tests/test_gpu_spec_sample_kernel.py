"""eetq_spec_sample_accept_f16 on the GPU (ops.spec_sample_accept) against tests/spec_sample_ref.py.  Integers
throughout: every comparison is exact.

* With the kernel's own random numbers the oracle of step 1 is the already-tested ``ops.sample_handover`` on ``logits[:, j]`` at
  column col + j (the contract's words); the reference then walks and hands over those tokens.
* With served random numbers the oracle is the float64 reference (tests/sampling_ref.py), u at the midpoints of reference
  intervals wider than test_gpu_sample.py's WIDE, its MARGIN asserted on every interval and on every top_p.
* At temperature 0 without EOS every output is ``ops.spec_accept``'s.
Logits as test_gpu_sample.py's ``_rows`` makes them; output and history are filled with sentinels, and every sentinel must survive."""
import numpy as np
import pytest
import torch

import sampling_ref
import spec_sample_ref as ref
from test_gpu_sample import MARGIN, WIDE, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILTERS = [(0, 1.0), (50, 1.0), (0, 0.9), (50, 0.9)]
ORDER = ("out_tokens", "column", "next_token", "position", "limit", "hist", "stats")


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    return o


def _logits(V, B, k, seed, sliced=False):
    """[B, k + 1, V] fp16 on the host and the device; ``sliced``: the [:, :, 1:] view, rows on 2-byte boundaries"""
    host = _rows(V, B * (k + 1), seed).reshape(B, k + 1, V)
    dev = torch.from_numpy(host).to(DEV)
    return (host[:, :, 1:], dev[:, :, 1:]) if sliced else (host, dev)


def _state(B, col=2, pos=40, limit=1000, out_cols=40, hist_cols=64):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=DEV)
    full = lambda shape, v: torch.full(shape, v, dtype=torch.int64, device=DEV)
    return dict(out_tokens=full((B, out_cols), -7), column=i64([[col]]), next_token=full((B, 1), -1), position=i64([pos]),
                limit=i64([limit]), hist=full((B, hist_cols), -9), stats=i64([3, 11]))


def _host(st):
    return {key: int(v) if key in ("column", "position", "limit") else v.cpu().numpy() for key, v in st.items()}


def _run_and_check(ops, lg, x, draft, st, params, what, done=None, uniforms=None, eos=-1, pad=0, workspace=None, mod=None):
    """one launch on the state ``st``; everything it may write against the reference fed the tokens ``x``; returns adv"""
    before = _host(st)
    done_before = None if done is None else done.cpu().numpy()
    want = ref.spec_sample_accept_ref(x, draft, eos_token=eos, pad_token=pad, done=done_before, **before)
    d = torch.from_numpy(np.ascontiguousarray(draft)).to(DEV)
    (mod or ops).spec_sample_accept(lg, d, *[st[key] for key in ORDER], params, done, uniforms, workspace)
    after = _host(st)
    out, col, tok, pos, hist, stats, done_want, adv = want
    assert after["column"] == col and after["position"] == pos and after["limit"] == before["limit"], (what, after, col, pos, adv)
    assert np.array_equal(after["out_tokens"], out), (what, adv, after["out_tokens"], out)
    assert np.array_equal(after["hist"], hist), (what, adv)
    assert np.array_equal(after["next_token"], tok), (what, adv, after["next_token"], tok)
    assert after["stats"].tolist() == stats.tolist(), (what, adv)
    if done is not None:
        assert done.cpu().numpy().tolist() == done_want.tolist(), (what, adv, done, done_want)
    assert torch.equal(d.cpu(), torch.from_numpy(np.ascontiguousarray(draft)))
    return adv


def _oracle(ops, lg, col, **settings):
    """x[b][j] = the token ops.sample_handover produces for logits[:, j] at column col + j (no EOS handling)"""
    B, T, _ = lg.shape
    params = ops.sampling_params(device=DEV, **settings)
    toks = []
    for j in range(T):
        out = torch.full((B, 1), -7, dtype=torch.int64, device=DEV)
        c = torch.tensor([[col + j]], dtype=torch.int64, device=DEV)
        tok = torch.full((B, 1), -1, dtype=torch.int64, device=DEV)
        pos = torch.zeros(1, dtype=torch.int64, device=DEV)
        ops.sample_handover(lg[:, j], out, c, tok, pos, params)
        toks.append(tok)
    return torch.cat(toks, dim=1).cpu().numpy()


def _drafts(x, V):
    """the draft that copies the oracle, then drafts made wrong for one row at each position in turn"""
    B, T = x.shape
    yield "right", x[:, :T - 1].copy()
    for j in range(T - 1):
        d = x[:, :T - 1].copy()
        d[j % B, j] = (d[j % B, j] + 1) % V
        yield "wrong at %d" % j, d


@pytest.mark.parametrize("V,B,k,sliced", [(7, 1, 1, False), (7, 3, 15, False), (1001, 3, 4, False), (1001, 3, 4, True),
                                          (1001, 1, 15, False), (32000, 3, 4, False), (32000, 1, 15, False)])
def test_own_random_numbers_exact(ops, V, B, k, sliced):
    host, lg = _logits(V, B, k, seed=V + 10 * B + k, sliced=sliced)
    Vv = host.shape[2]
    ws = torch.empty(B * (k + 1), dtype=torch.int64, device=DEV)
    for T in (0.5, 1.7):
        for top_k, top_p in FILTERS:
            settings = dict(temperature=T, top_k=top_k, top_p=top_p, seed=1234 + top_k)
            col = 2
            x = _oracle(ops, lg, col, **settings)
            assert x.min() >= 0 and x.max() < Vv
            params = ops.sampling_params(device=DEV, **settings)
            for name, draft in _drafts(x, Vv):
                adv = _run_and_check(ops, lg, x, draft, _state(B, col=col), params, (V, B, k, sliced, T, top_k, top_p, name), workspace=ws)
                assert adv == (k + 1 if name == "right" else int(name.split()[-1]) + 1)


def _served(host, T, top_k, top_p):
    """per (b, t): the float64 reference's token and a u at the midpoint of one of its wide intervals (which one varies)"""
    B, Tn, _ = host.shape
    x = np.zeros((B, Tn), dtype=np.int64)
    u = np.zeros((B, Tn), dtype=np.float32)
    for b in range(B):
        for t in range(Tn):
            r = sampling_ref.sample_row(host[b, t], T, top_k=top_k, top_p=top_p)
            assert r.special is None and r.p_margin >= MARGIN, (b, t, T, top_k, top_p, r.p_margin)
            wide = np.nonzero(r.hi - r.lo > WIDE)[0]
            assert wide.size >= 1
            i = wide[(3 * b + t) % wide.size]
            u[b, t] = np.float32((r.lo[i] + r.hi[i]) / 2)
            assert u[b, t] - r.lo[i] >= MARGIN and r.hi[i] - u[b, t] >= MARGIN
            x[b, t] = r.order[i]
    return x, u


SERVED = [(7, 3, 4, False, 23), (1001, 3, 4, False, 2), (1001, 3, 4, True, 2), (1001, 1, 15, False, 3), (32000, 3, 1, False, 4),
          (32000, 1, 4, False, 5)]


@pytest.mark.parametrize("V,B,k,sliced,seed", SERVED)
def test_served_uniforms_against_float64(ops, V, B, k, sliced, seed):
    host, lg = _logits(V, B, k, seed=seed, sliced=sliced)
    Vv = host.shape[2]
    for T in (0.5, 1.7):
        for top_k, top_p in FILTERS:
            x, u = _served(host, T, top_k, top_p)
            assert np.array_equal(x, ref.draw_tokens(host, 2, k + 1, temperature=T, top_k=top_k, top_p=top_p, uniforms=u))
            params = ops.sampling_params(temperature=T, top_k=top_k, top_p=top_p, seed=77, device=DEV)
            ud = torch.from_numpy(u).to(DEV)
            wrong = x[:, :k].copy()
            wrong[B - 1, k // 2] = (wrong[B - 1, k // 2] + 1) % Vv
            for name, draft in (("right", x[:, :k]), ("wrong", wrong)):
                adv = _run_and_check(ops, lg, x, draft, _state(B), params, (V, B, k, sliced, T, top_k, top_p, name), uniforms=ud)
                assert adv == (k + 1 if name == "right" else k // 2 + 1)
    # a wider uniforms tensor: the row stride is the tensor's, not k + 1 (B > 1 only: one row has no stride to speak of)
    if B > 1:
        wide = torch.full((B, k + 4), 2.0, dtype=torch.float32, device=DEV)
        wide[:, :k + 1] = ud
        assert _run_and_check(ops, lg, x, x[:, :k], _state(B), params, "strided uniforms", uniforms=wide[:, :k + 1]) == k + 1


def test_temperature_zero_is_spec_accept(ops):
    """T = 0 (and negative, and NaN), no EOS, done=None: every output equals ops.spec_accept's on the same inputs"""
    import eetq_amd.ops_ctypes as ops_ctypes
    torch.manual_seed(5)
    for B, k, V in ((1, 4, 32000), (3, 4, 1001), (3, 15, 7), (1, 1, 1001)):
        lg = (torch.randn(B, k + 1, V, device=DEV) * 3).half()
        if V > 100:
            lg[0, 0, 17] = lg[0, 0, 90] = lg[0, 0].max() + 1                     # a tie: the first index
            lg[B - 1, 1, 5] = float("nan")                                       # a NaN is the maximum
            lg[B - 1, 1, 3] = float("inf")
        else:
            lg[0, 0] = 0.0
            lg[0, 0, 2] = -0.0
        for view in (lg, lg[:, :, 1:]):
            g = view.argmax(-1)
            for T in (0.0, -1.0, float("nan")):
                params = ops.sampling_params(temperature=T, top_k=5, top_p=0.5, device=DEV)
                for j in (None, 0, k - 1):
                    for limit in (1000, 2 + k):
                        draft = g[:, :k].clone()
                        if j is not None:
                            draft[B - 1, j] = (draft[B - 1, j] + 1) % view.shape[2]
                        a, b = _state(B, limit=limit), _state(B, limit=limit)
                        ops.spec_accept(view, draft, *[a[key] for key in ORDER])
                        mod = ops_ctypes if (j == 0 and T == 0.0) else ops
                        mod.spec_sample_accept(view, draft, *[b[key] for key in ORDER], params)      # workspace=None: allocated
                        for key in ORDER:
                            assert torch.equal(a[key], b[key]), (B, k, V, T, j, limit, key)
                        adv = min(k + 1 if j is None else j + 1, k)                                  # limit - column = k
                        assert int(b["column"]) == 2 + (adv if limit == 2 + k else (k + 1 if j is None else j + 1))
    with pytest.raises(RuntimeError):
        ops.spec_sample_accept(lg.float(), draft, *[a[key] for key in ORDER], params)
    with pytest.raises(RuntimeError):
        ops.spec_sample_accept(lg, draft, *[a[key] for key in ORDER], params.long())
    with pytest.raises(RuntimeError):
        ops.spec_sample_accept(lg, draft, *[a[key] for key in ORDER], params, None, None, torch.empty(1, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("B,k", [(1, 4), (3, 4), (3, 1)])
def test_limit(ops, B, k):
    V, col = 1001, 5
    host, lg = _logits(V, B, k, seed=31 + B + k)
    settings = dict(temperature=1.3, top_k=50, top_p=0.9, seed=99)
    x = _oracle(ops, lg, col, **settings)
    params = ops.sampling_params(device=DEV, **settings)
    wrong = x[:, :k].copy()
    wrong[0, k - 1] = (wrong[0, k - 1] + 1) % V
    for room in (-1, 0, 1, k, k + 1, k + 5):
        for name, draft, n in (("right", x[:, :k], k + 1), ("wrong", wrong, k)):
            done = torch.zeros(B, dtype=torch.int32, device=DEV)
            adv = _run_and_check(ops, lg, x, draft, _state(B, col=col, limit=col + room), params, (B, k, room, name), done=done)
            assert adv == max(0, min(room, n))


def test_eos_and_done(ops):
    """T = 0: the tokens are the argmaxes, known on the CPU (distinct head logits: no ties), so every scenario is checked
    on the CPU before it is run."""
    B, k, V, pad = 3, 4, 1001, 77
    host, lg = _logits(V, B, k, seed=8)
    x = host.astype(np.float32).argmax(-1)
    assert len(set(x.reshape(-1).tolist())) == B * (k + 1)                     # all different: an EOS token hits one place only
    right = x[:, :k].copy()

    def run(draft, eos, done_in, what, **kw):
        params = ops.sampling_params(temperature=0.0, eos_token_id=eos, pad_token_id=pad, device=DEV)
        done = torch.tensor(done_in, dtype=torch.int32, device=DEV)
        st = _state(B, **kw)
        adv = _run_and_check(ops, lg, x, draft, st, params, what, done=done, eos=-1 if eos is None else eos, pad=pad)
        return adv, st, done.tolist()

    # a row flagged at entry hands on pads and never objects (its draft is wrong everywhere; its logits are not looked at)
    d = right.copy()
    d[1] = (d[1] + 1) % V
    nan_lg = lg.clone()
    nan_lg[1] = float("nan")
    adv, st, done = run(d, None, [0, 1, 0], "flagged at entry")
    assert adv == k + 1 and done == [0, 1, 0] and (st["out_tokens"][1, 2:2 + k + 1] == pad).all() and int(st["next_token"][1]) == pad
    params = ops.sampling_params(temperature=0.0, pad_token_id=pad, device=DEV)
    dn = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    assert _run_and_check(ops, nan_lg, x, d, _state(B), params, "flagged, NaN logits", done=dn, pad=pad) == k + 1
    # a row that draws EOS at j < adv is flagged, pads after it, and its later draft mismatches do not end the step
    d = right.copy()
    d[2, 2:] = (d[2, 2:] + 1) % V
    adv, st, done = run(d, int(x[2, 1]), [0, 0, 0], "EOS at 1")
    assert adv == k + 1 and done == [0, 0, 1]
    assert st["out_tokens"][2, 2:2 + k + 1].tolist() == [int(x[2, 0]), int(x[2, 1])] + [pad] * (k - 1)
    # an EOS at position adv - 1 finishes its row; one at a position >= adv leaves done at 0
    d = right.copy()
    d[0, 1] = (d[0, 1] + 1) % V                                                # row 0 objects at position 1: adv = 2
    adv, st, done = run(d, int(x[1, 1]), [0, 0, 0], "EOS at adv - 1")
    assert adv == 2 and done == [0, 1, 0]
    adv, st, done = run(d, int(x[1, 2]), [0, 0, 0], "EOS beyond adv")
    assert adv == 2 and done == [0, 0, 0]
    adv, st, done = run(d, int(x[1, 3]), [0, 0, 0], "EOS beyond the limit", limit=3)       # want = 1
    assert adv == 1 and done == [0, 0, 0]
    # every row finished: adv = want, whatever the draft
    adv, st, done = run((right + 1) % V, int(x[0, 0]), [1, 1, 1], "all finished")
    assert adv == k + 1 and done == [1, 1, 1] and (st["out_tokens"][:, 2:2 + k + 1] == pad).all()
    adv, st, done = run((right + 1) % V, int(x[0, 0]), [1, 1, 1], "all finished, clamped", limit=5)
    assert adv == 3
    # done=None: no row is finished at entry; an EOS of this step still pads the positions behind it
    params = ops.sampling_params(temperature=0.0, eos_token_id=int(x[2, 0]), pad_token_id=pad, device=DEV)
    st = _state(B)
    assert _run_and_check(ops, lg, x, (right + 1) % V, st, params, "done=None", eos=int(x[2, 0]), pad=pad) == 1
    d = right.copy()
    d[2] = (d[2] + 1) % V
    st = _state(B)
    assert _run_and_check(ops, lg, x, d, st, params, "done=None, EOS at 0", eos=int(x[2, 0]), pad=pad) == k + 1
    assert st["out_tokens"][2, 2:2 + k + 1].tolist() == [int(x[2, 0])] + [pad] * k


def test_sampled_eos(ops):
    """a SAMPLED draw of the EOS token: served numbers, the float64 reference's tokens"""
    B, k, V, pad = 3, 4, 1001, 5
    host, lg = _logits(V, B, k, seed=2)
    x, u = _served(host, 1.7, 50, 0.9)
    ud = torch.from_numpy(u).to(DEV)
    for row, j in ((0, 0), (1, 2), (2, k)):
        eos = int(x[row, j])
        params = ops.sampling_params(temperature=1.7, top_k=50, top_p=0.9, eos_token_id=eos, pad_token_id=pad, device=DEV)
        done = torch.zeros(B, dtype=torch.int32, device=DEV)
        adv = _run_and_check(ops, lg, x, x[:, :k], _state(B), params, ("sampled EOS", row, j), done=done, uniforms=ud, eos=eos, pad=pad)
        assert adv == k + 1 and done[row] == 1


def test_ticket(ops):
    """48 workgroups count themselves in bits 40.. of *position: it comes out as position + adv exactly, from a negative
    position, from 0 and from just below 2^39, and the column as column + adv"""
    B, k, V = 3, 15, 1001
    assert B * (k + 1) == 48
    host, lg = _logits(V, B, k, seed=12)
    settings = dict(temperature=1.0, seed=5)
    x = _oracle(ops, lg, 7, **settings)
    params = ops.sampling_params(device=DEV, **settings)
    ws = torch.empty(48, dtype=torch.int64, device=DEV)
    for start in (-5, 0, 2 ** 39 - 64):
        for name, draft in list(_drafts(x, V))[::5]:
            st = _state(B, col=7, pos=start)
            adv = _run_and_check(ops, lg, x, draft, st, params, (start, name), workspace=ws)
            assert int(st["position"]) == start + adv and int(st["column"]) == 7 + adv and adv >= 1
        st = _state(B, col=7, pos=start, limit=7)                               # adv = 0: the tickets are taken out all the same
        assert _run_and_check(ops, lg, x, x[:, :k], st, params, (start, "adv 0"), workspace=ws) == 0 and int(st["position"]) == start


def test_three_steps_under_one_graph_replay(ops):
    """served logits, the column advances inside the graph: each step's tokens are those of its own columns"""
    B, k, V = 2, 4, 1001
    host, lg0 = _logits(V, B, k, seed=6)
    lg = torch.zeros_like(lg0)
    params = ops.sampling_params(temperature=1.0, seed=3, device=DEV)
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    st = _state(B, col=0, limit=0)
    draft = torch.zeros(B, k, dtype=torch.int64, device=DEV)
    ws = torch.empty(B * (k + 1), dtype=torch.int64, device=DEV)
    call = lambda: ops.spec_sample_accept(lg, draft, *[st[key] for key in ORDER], params, done, None, ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                                  # warm-up outside the capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(3):
                call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for T, top_k, seed, eos_at in ((1.3, 40, 11, None), (0.8, 0, 12, (1, 1))):   # rewritten logits, parameters, flags: no recapture
        settings = dict(temperature=T, top_k=top_k, seed=seed)
        lg.copy_(lg0)
        col, pos = 1, 9
        x0 = _oracle(ops, lg, col, **settings)
        eos = None if eos_at is None else int(x0[eos_at])
        ops.sampling_params(eos_token_id=eos, pad_token_id=5, out=params, **settings)
        draft.copy_(torch.from_numpy(x0[:, :k]))                                # right at the first step's columns
        fresh = _state(B, col=col, pos=pos)
        for key in ORDER:
            st[key].copy_(fresh[key])
        done.zero_()
        graph.replay()
        torch.cuda.synchronize()
        e = _host(fresh)
        e_done = np.zeros(B, dtype=np.int32)
        advs = []
        for _ in range(3):
            x = _oracle(ops, lg, e["column"], **settings)
            out, c, tok, p, hist, stats, e_done, adv = ref.spec_sample_accept_ref(x, x0[:, :k], eos_token=-1 if eos is None else eos,
                                                                                  pad_token=5, done=e_done, **e)
            e.update(out_tokens=out, column=c, next_token=tok, position=p, hist=hist, stats=stats)
            advs.append(adv)
        got = _host(st)
        assert advs[0] == k + 1 and got["column"] == col + sum(advs) and got["position"] == pos + sum(advs), (advs, got)
        for key in ("out_tokens", "next_token", "hist", "stats"):
            assert np.array_equal(got[key], e[key]), (key, advs)
        assert done.cpu().numpy().tolist() == e_done.tolist()
        if eos is not None:
            assert done[eos_at[0]] == 1
