"""``GraphDecoder(speculative=k)``: speculative greedy decoding by n-gram lookup, captured and eager, on the tiny accelerated
Llama of tests/test_gpu_multiturn.py (hidden 256, 4 heads / 2 KV heads of 64, 2 layers, vocab 512), 96 cache rows, k = 4.

* The CYCLE model has zero output and down projections, so the hidden state is the token's embedding, and an lm_head whose row
  perm[t] is the embedding of t: the greedy token after t is perm[t], whatever the attention does.  Its tokens are known on
  the CPU (the orbit of perm) and, once the prompt holds a full cycle, every lookup draft is right.
* The RANDOM model is the multi-turn test's.  A verify pass computes a token's logits with the prompt kernels where a plain
  step uses the decode kernels, so token equality with the plain decoder is not demanded (a near-tie may flip).  Demanded is
  that EVERY emitted token is an argmax, within tolerance, of the same model run once over the finished sequence without a
  cache: rowmax - logit[token] <= 2 * (4e-3 * max|logits| + 4e-3), test_gpu_multiturn.py's logit tolerance once for each of the
  two logits compared."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN, K, VOCAB = 96, 4, 512


@pytest.fixture(scope="module")
def cfg():
    transformers = pytest.importorskip("transformers")
    return transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4,
                                    num_key_value_heads=2, vocab_size=VOCAB, max_position_embeddings=128)


def _accelerate(stock):
    from eetq_amd.utils import eet_accelerator
    return eet_accelerator(copy.deepcopy(stock), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)


@pytest.fixture(scope="module")
def stock(cfg):
    import transformers
    torch.manual_seed(0)
    return transformers.LlamaForCausalLM(cfg).half().to(DEV).eval()


@pytest.fixture(scope="module")
def model(stock):
    return _accelerate(stock)


@pytest.fixture(scope="module")
def perm():
    """a permutation of the vocabulary with two 7-cycles (10 .. 16 and 20 .. 26, in a shuffled order each)"""
    g = torch.Generator().manual_seed(3)
    p = torch.arange(VOCAB)
    rest = torch.tensor([t for t in range(VOCAB) if not (10 <= t < 17 or 20 <= t < 27)])
    p[rest] = rest[torch.randperm(len(rest), generator=g)]
    for lo in (10, 20):
        cyc = lo + torch.randperm(7, generator=g)
        p[cyc] = cyc.roll(-1)
    return p


@pytest.fixture(scope="module")
def cycle_model(cfg, perm):
    import transformers
    torch.manual_seed(1)
    m = transformers.LlamaForCausalLM(cfg).half().to(DEV).eval()
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.o_proj.weight.zero_()
            layer.mlp.down_proj.weight.zero_()
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(VOCAB)
        m.lm_head.weight.copy_(m.model.embed_tokens.weight[inv.to(DEV)])        # row v = the embedding of perm^-1[v]
    return _accelerate(m)


def _orbit(perm, start, n):
    out, t = [], int(start)
    for _ in range(n):
        t = int(perm[t])
        out.append(t)
    return out


def _counters(cache):
    return [int(layer.cumulative_length) for layer in cache.layers]


def _decoder(model, batch, capture=True, **kw):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(model, batch, MAX_LEN, capture=capture, speculative=K, **kw)


@pytest.fixture(scope="module")
def cycle_decoders(cycle_model):
    return {(b, cap): _decoder(cycle_model, b, capture=cap) for b in (1, 2) for cap in (True, False)}


@pytest.mark.parametrize("capture", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("batch", [1, 2])
def test_cycle_model_tokens_and_accepted_drafts(cycle_decoders, perm, batch, capture):
    dec = cycle_decoders[(batch, capture)]
    rows = []
    for b, first in enumerate((10, 23)[:batch]):
        rows.append([first] + _orbit(perm, first, 8))                             # 9 tokens: a full cycle and two more
    prompt = torch.tensor(rows, device=DEV)
    for new in (1, 2, 5, 6, 23):
        got = dec.generate(prompt, new)
        want = [r + _orbit(perm, r[-1], new) for r in rows]
        assert got.tolist() == want, (new, got.tolist(), want)
        steps, tokens = dec.spec_stats()
        assert tokens == new - 1 and steps <= -(-new // (K + 1)) + 2, (new, steps, tokens)
        assert dec.rows == 9 + new - 1 and _counters(dec.cache) == [dec.rows] * 2 and int(dec.s_pos) == dec.rows
        assert dec.s_hist[:, :9 + new].tolist() == want and int(dec.s_tok[0, 0]) == want[0][-1]


def test_cycle_model_drafts_are_what_is_accepted(cycle_decoders, perm):
    """23 tokens in ceil(22 / 5) = 5 verify steps: every one of them handed over k + 1 tokens but the clamped last"""
    dec = cycle_decoders[(1, True)]
    prompt = torch.tensor([[10] + _orbit(perm, 10, 8)], device=DEV)
    dec.generate(prompt, 23)
    assert dec.spec_stats() == (5, 22)
    # a prompt without a repetition: the first steps reject, the cycle is found once the sequence itself holds it
    got = dec.generate(prompt[:, :3], 30)
    assert got.tolist() == [prompt[0, :3].tolist() + _orbit(perm, int(prompt[0, 2]), 30)]
    steps, tokens = dec.spec_stats()
    assert tokens == 29 and 6 <= steps < 29


def _tol(ref):
    return 4e-3 * ref.abs().max().item() + 4e-3


def _assert_every_token_is_an_argmax(model, seq, generated, what):
    """seq [B, S]: the finished sequence; generated: the columns the decoder emitted.  One pass without a cache."""
    with torch.no_grad():
        logits = model(seq[:, :-1]).logits.float()
    tol = 2 * _tol(logits)
    worst = 0.0
    for c in generated:
        row = logits[:, c - 1]
        gap = row.max(-1).values - row.gather(1, seq[:, c:c + 1])[:, 0]
        worst = max(worst, gap.max().item())
    print("spec decoder %s: %d columns, worst rowmax - logit[token] %.3g of %.3g" % (what, len(generated), worst, tol))
    assert worst <= tol, (what, worst, tol)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(11)
    return (torch.randint(0, VOCAB, (2, 9), generator=g).to(DEV), torch.randint(0, VOCAB, (2, 5), generator=g).to(DEV))


@pytest.fixture(scope="module")
def spec(model):
    return _decoder(model, 2)


@pytest.fixture(scope="module")
def plain(model):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(model, 2, MAX_LEN)


def test_random_model_lookup_drafts(model, spec, prompts):
    """(a) lookup drafts on a random model are mostly rejected: the rollback path, step after step"""
    seq = spec.generate(prompts[0], 40)
    steps, tokens = spec.spec_stats()
    assert tokens == 39 and 8 <= steps <= 39 and spec.rows == 48 and _counters(spec.cache) == [48, 48]
    assert torch.equal(spec.s_hist[:, :49], seq)
    _assert_every_token_is_an_argmax(model, seq, range(9, 49), "lookup drafts (%d steps for 39 tokens)" % steps)


def test_random_model_served_drafts(model, plain, prompts):
    """(b) eager, with a draft hook that serves the first j tokens of the plain decoder's continuation and then wrong ones,
    j cycling 0 .. k: accepts of every length and rejects at every position"""
    new = 40
    cont = plain.generate(prompts[0], new + K)[:, 9:]
    calls = [0]

    def draft(dec):
        i = int(dec.s_idx)                        # tokens emitted so far: the pending one is cont[:, i - 1] if nothing diverged
        j = calls[0] % (K + 1)
        calls[0] += 1
        d = cont[:, i:i + K].clone()
        d[:, j:] = (d[:, j:] + 1) % VOCAB
        return d

    dec = _decoder(model, 2, capture=False, draft=draft)
    seq = dec.generate(prompts[0], new)
    steps, tokens = dec.spec_stats()
    assert steps == calls[0] and tokens == new - 1 and tokens > steps, (steps, tokens)
    assert steps > -(-(new - 1) // (K + 1))                                         # ... and rejects happened
    _assert_every_token_is_an_argmax(model, seq, range(9, 9 + new), "served drafts (%d steps for %d tokens)" % (steps, tokens))


def test_random_model_two_turns(model, spec, prompts):
    """(c) a second turn behind the first: the pending token and the prompt go behind the cached rows, the history follows"""
    t1 = spec.generate(prompts[0], 12)
    assert spec.rows == 9 + 12 - 1
    t2 = spec.generate(prompts[1], 14, append=True)
    assert t2.shape == (2, 19) and torch.equal(t2[:, :5], prompts[1])
    whole = torch.cat([t1, t2], dim=1)
    assert spec.rows == 39 and _counters(spec.cache) == [39, 39] and torch.equal(spec.s_hist[:, :40], whole)
    _assert_every_token_is_an_argmax(model, whole, list(range(9, 21)) + list(range(26, 40)), "two turns")


def test_speculate_false_is_the_plain_decoder(spec, plain, prompts):
    """(d) the plain graphs of a speculative decoder are the plain decoder's; the history is kept for a later speculative turn"""
    a = spec.generate(prompts[0], 20, speculate=False)
    b = plain.generate(prompts[0], 20)
    assert torch.equal(a, b) and spec.spec_stats() == (0, 0)
    assert torch.equal(spec.s_hist[:, :29], a) and spec.rows == plain.rows == 28 and _counters(spec.cache) == [28, 28]
    c = spec.generate(prompts[1], 6, append=True)                  # speculative again, behind the plain turn
    assert c.shape == (2, 11) and spec.spec_stats()[1] == 5 and torch.equal(spec.s_hist[:, 29:40], c)


def test_refusals(model, stock, plain, prompts):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    with pytest.raises(ValueError, match="ragged=True"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, ragged=True)
    with pytest.raises(ValueError, match="greedy verification only"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, sampling=True)
    with pytest.raises(ValueError, match="fp16 cache rows"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, kv_bits=8)
    with pytest.raises(ValueError, match="lean=True"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, lean=False)
    with pytest.raises(ValueError, match="fully accelerated model"):
        GraphDecoder(stock, 2, MAX_LEN, speculative=K)
    for bad in (-1, 16, 2.0, True):
        with pytest.raises(ValueError, match="speculative must be"):
            GraphDecoder(model, 2, MAX_LEN, speculative=bad)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="ngram must lie"):
            GraphDecoder(model, 2, MAX_LEN, speculative=K, ngram=bad)
    with pytest.raises(ValueError, match="cache rows per verify step"):
        GraphDecoder(model, 2, K, speculative=K)
    with pytest.raises(ValueError, match="speculative decoder"):
        GraphDecoder(model, 2, MAX_LEN, draft=lambda dec: None)
    # a default decoder: no speculative state, the graphs it always had, and no speculative generate
    assert plain.speculative == 0 and plain.graph is not None and plain.graph_n is not None and plain.graph_spec is None
    for name in ("s_hist", "s_draft", "s_limit", "s_stats"):
        assert not hasattr(plain, name)
    with pytest.raises(ValueError, match="speculative=k"):
        plain.generate(prompts[0], 4, speculate=True)
    with pytest.raises(ValueError, match="speculative=k"):
        plain.spec_stats()
    assert torch.equal(plain.generate(prompts[0], 4, speculate=False), plain.generate(prompts[0], 4))


def test_spare_rows(spec, prompts):
    """fed + new + k <= max_len: a verify pass writes up to k rows past the last kept one"""
    with pytest.raises(ValueError, match="spare cache rows"):
        spec.generate(prompts[0], MAX_LEN - 9 - K + 1)
    out = spec.generate(prompts[0], MAX_LEN - 9 - K)                # the longest call that fits
    assert out.shape == (2, MAX_LEN - K) and spec.rows == MAX_LEN - K - 1
    assert spec.generate(prompts[0], MAX_LEN - 9, speculate=False).shape == (2, MAX_LEN)   # the plain graphs need none
