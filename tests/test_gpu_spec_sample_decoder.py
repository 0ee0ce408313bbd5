"""``GraphDecoder(speculative=k, sampling=True, spec_sampling=True)``: speculative decoding for sampled generation (DESIGN.md
4.17), captured and eager, k = 4, batch 1 and 2, on the CYCLE model of tests/test_gpu_spec_decoder.py rebuilt here: zero output
and down projections and an lm_head whose row perm[t] is the embedding of t, so the hidden state is the token's embedding and the
top token after t is perm[t], by a wide margin, whatever the attention does.

Sampled tokens are checked WITHOUT demanding equality with another decoder (a verify pass computes a token's logits with the prompt
kernels, a plain step with the decode kernels).  The sampler walks the classes by value descending, so the top token is drawn
iff u < p_top, u = Philox(seed; column, row) -- known on the CPU.  With R = (1 - p_top) / p_top from the same model run once over
the finished sequence without a cache, and every logit off by at most eps = twice test_gpu_spec_decoder.py's logit tolerance (once
for each of the two logits compared), the decoder's own R lies within R e^(+-2 eps / T): the emitted token MUST be perm[prev]
when u < 1 / (1 + R e^(2 eps / T)) and MUST differ when u > 1 / (1 + R e^(-2 eps / T)); columns inside the band are left out, at
most 5 % of them."""
import copy
import math

import numpy as np
import pytest
import torch

from sampling_ref import philox_uniform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN, K, VOCAB = 96, 4, 512
TEMPERATURE = 0.6      # chosen on the CPU (test_temperature_choice): mean p_top 0.890 over the vocabulary (0.759 .. 0.961)
SEED = 173             # chosen on the CPU with that restatement: both rows stay on their cycles for the first 10 columns (accepted
                       # drafts), both jump later, and no u of the first 80 columns comes closer than 0.009 to a band's edge


@pytest.fixture(scope="module")
def cfg():
    transformers = pytest.importorskip("transformers")
    return transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4,
                                    num_key_value_heads=2, vocab_size=VOCAB, max_position_embeddings=128)


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
def cycle_cpu(cfg, perm):
    """the CYCLE model on the CPU, fp16 weights"""
    import transformers
    torch.manual_seed(1)
    m = transformers.LlamaForCausalLM(cfg).half().eval()
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.o_proj.weight.zero_()
            layer.mlp.down_proj.weight.zero_()
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(VOCAB)
        m.lm_head.weight.copy_(m.model.embed_tokens.weight[inv])          # row v = the embedding of perm^-1[v]
    return m


@pytest.fixture(scope="module")
def cycle_model(cycle_cpu):
    from eetq_amd.utils import eet_accelerator
    return eet_accelerator(copy.deepcopy(cycle_cpu).to(DEV), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True,
                           fused_residual=True)


def _tol(ref):
    return 4e-3 * ref.abs().max().item() + 4e-3       # test_gpu_spec_decoder.py's logit tolerance


def _band(p_top, eps, T):
    """(must be the top token below, must differ above) for a top-token probability and a logit error bound"""
    R = (1.0 - p_top) / p_top
    return 1.0 / (1.0 + R * math.exp(2 * eps / T)), 1.0 / (1.0 + R * math.exp(-2 * eps / T))


def test_temperature_choice(cycle_cpu, cfg, perm):
    """The float32 restatement of the CYCLE model: logits(t) = lm_head . rmsnorm(embedding of t).  At T = 0.6 the top token's
    probability is 0.890 on average over the vocabulary (0.759 .. 0.961): jumps and accepted drafts both occur.  The band
    is 0.034 wide on average (eps from the restatement's own logits), under the 5 % of columns that may be left out."""
    emb = cycle_cpu.model.embed_tokens.weight.float()
    n = emb * torch.rsqrt((emb * emb).mean(-1, keepdim=True) + cfg.rms_norm_eps) * cycle_cpu.model.norm.weight.float()
    logits = n @ cycle_cpu.lm_head.weight.float().T
    assert torch.equal(logits.argmax(-1), perm)
    p_top = torch.softmax(logits / TEMPERATURE, -1)[torch.arange(VOCAB), perm]
    print("cycle model at T = %.2f: p_top mean %.3f, min %.3f, max %.3f" % (TEMPERATURE, p_top.mean().item(), p_top.min().item(),
                                                                            p_top.max().item()))
    assert 0.85 <= p_top.mean().item() <= 0.95
    eps = 2 * _tol(logits)
    width = np.mean([hi - lo for lo, hi in (_band(p, eps, TEMPERATURE) for p in p_top.tolist())])
    print("band: eps %.3g, mean width %.4f" % (eps, width))
    assert width < 0.05


def _orbit(perm, start, n):
    out, t = [], int(start)
    for _ in range(n):
        t = int(perm[t])
        out.append(t)
    return out


def _counters(cache):
    return [int(layer.cumulative_length) for layer in cache.layers]


def _prompt(perm, batch):
    rows = [[first] + _orbit(perm, first, 8) for first in (10, 23)[:batch]]      # 9 tokens: a full cycle and two more
    return rows, torch.tensor(rows, device=DEV)


@pytest.fixture(scope="module")
def decoders(cycle_model):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    cache = {}

    def get(batch, capture, spec=True):
        key = (batch, capture, spec)
        if key not in cache:
            kw = dict(speculative=K, spec_sampling=True) if spec else {}
            cache[key] = GraphDecoder(cycle_model, batch, MAX_LEN, capture=capture, sampling=True, **kw)
        return cache[key]
    return get


CASES = pytest.mark.parametrize("batch,capture", [(1, True), (2, True), (1, False), (2, False)],
                                ids=["b1-captured", "b2-captured", "b1-eager", "b2-eager"])


@CASES
def test_greedy_tokens_are_the_orbit(decoders, perm, batch, capture):
    dec = decoders(batch, capture)
    rows, prompt = _prompt(perm, batch)
    for new in (1, 2, 5, 6, 23):
        got = dec.generate(prompt, new)                                          # do_sample=False
        want = [r + _orbit(perm, r[-1], new) for r in rows]
        assert got.tolist() == want, (new, got.tolist(), want)
        steps, tokens = dec.spec_stats()
        assert tokens == new - 1 and steps <= -(-new // (K + 1)) + 2, (new, steps, tokens)
        assert dec.rows == 9 + new - 1 and _counters(dec.cache) == [dec.rows] * 2 and int(dec.s_pos) == dec.rows
        assert dec.s_hist[:, :9 + new].tolist() == want and int(dec.s_tok[0, 0]) == want[0][-1]
        assert dec.done.tolist() == [0] * batch
    dec.generate(prompt, 23)
    assert dec.spec_stats() == (5, 22)                                           # every draft accepted: ceil(22 / 5) steps


@CASES
def test_eos_stops_a_row(decoders, perm, batch, capture):
    dec = decoders(batch, capture)
    rows, prompt = _prompt(perm, batch)
    new, pad = 23, 3
    dec.generate(prompt, new)
    steps_without = dec.spec_stats()[0]
    orbit = [_orbit(perm, r[-1], new) for r in rows]
    eos = orbit[0][6]                                                            # a token of row 0's cycle only
    assert all(eos not in o for o in orbit[1:]) and orbit[0].index(eos) == 6
    got = dec.generate(prompt, new, eos_token_id=eos, pad_token_id=pad)
    assert got[0, 9:].tolist() == orbit[0][:7] + [pad] * (new - 7)
    if batch == 2:
        assert got[1, 9:].tolist() == orbit[1]                                   # row 1 still gets its orbit
    assert dec.done.tolist() == [1, 0][:batch]
    steps, tokens = dec.spec_stats()
    assert tokens == new - 1 and steps <= steps_without, (steps, steps_without)
    assert dec.rows == 9 + new - 1 and _counters(dec.cache) == [dec.rows] * 2


def _check_sampled(model, perm, seq, spans, seed, what, share=0.05):
    """seq [B, S]: the finished sequence; spans: (first generated column of seq, count) per generate call -- its Philox columns
    count from 0.  ``share``: the share of columns that may be left out (None: any).  Returns (columns checked, left out, jumps)."""
    with torch.no_grad():
        logits = model(seq[:, :-1]).logits.float()
    eps = 2 * _tol(logits)
    prob = torch.softmax(logits / TEMPERATURE, -1).cpu()
    seq = seq.cpu()
    checked = left_out = jumps = 0
    for first, count in spans:
        for c in range(count):
            for b in range(seq.shape[0]):
                prev, tok = int(seq[b, first + c - 1]), int(seq[b, first + c])
                top = int(perm[prev])
                lo, hi = _band(float(prob[b, first + c - 1, top]), eps, TEMPERATURE)
                u = float(philox_uniform(seed, c, b))
                jumps += tok != top
                if u < lo:
                    assert tok == top, (what, b, c, u, lo, hi, prev, tok, top)
                elif u > hi:
                    assert tok != top, (what, b, c, u, lo, hi, prev, tok, top)
                else:
                    left_out += 1
                    continue
                checked += 1
    total = checked + left_out
    print("spec sampling %s: %d columns, %d left out, %d jumps (eps %.3g)" % (what, total, left_out, jumps, eps))
    assert share is None or left_out <= share * total, (what, left_out, total)
    return checked, left_out, jumps


@CASES
def test_sampled_tokens(decoders, cycle_model, perm, batch, capture):
    """T = 0.6 (mean p_top 0.890, see test_temperature_choice), seed 173: the top token below the band, another one above it; at
    least one jump and at least one step that handed over several tokens"""
    dec = decoders(batch, capture)
    rows, prompt = _prompt(perm, batch)
    new = 80
    seq = dec.generate(prompt, new, do_sample=True, temperature=TEMPERATURE, seed=SEED)
    steps, tokens = dec.spec_stats()
    assert seq.shape == (batch, 9 + new) and tokens == new - 1 and int(seq.min()) >= 0 and int(seq.max()) < VOCAB
    assert dec.rows == 9 + new - 1 and _counters(dec.cache) == [dec.rows] * 2 and torch.equal(dec.s_hist[:, :9 + new], seq)
    checked, left_out, jumps = _check_sampled(cycle_model, perm, seq, [(9, new)], SEED, "b%d %s" % (batch, "captured" if capture else "eager"))
    assert jumps >= 1 and steps > -(-(new - 1) // (K + 1))                        # a jump, and the rejected draft it caused
    assert steps < tokens                                                        # a step that handed over several tokens
    # seeds: the same seed twice gives equal outputs, another seed different ones
    assert torch.equal(seq, dec.generate(prompt, new, do_sample=True, temperature=TEMPERATURE, seed=SEED))
    assert not torch.equal(seq, dec.generate(prompt, new, do_sample=True, temperature=TEMPERATURE, seed=SEED + 1))


@CASES
def test_speculate_false_is_the_plain_sampling_decoder(decoders, perm, batch, capture):
    dec, plain = decoders(batch, capture), decoders(batch, capture, spec=False)
    rows, prompt = _prompt(perm, batch)
    kw = dict(do_sample=True, temperature=TEMPERATURE, top_k=20, top_p=0.95, seed=SEED)
    a = dec.generate(prompt, 30, speculate=False, **kw)
    b = plain.generate(prompt, 30, **kw)
    assert torch.equal(a, b) and dec.spec_stats() == (0, 0)
    assert torch.equal(dec.s_hist[:, :39], a) and dec.rows == plain.rows == 38 and _counters(dec.cache) == [38, 38]


@CASES
def test_second_turn(decoders, cycle_model, perm, batch, capture):
    dec = decoders(batch, capture)
    rows, prompt = _prompt(perm, batch)
    kw = dict(do_sample=True, temperature=TEMPERATURE)
    t1 = dec.generate(prompt, 12, seed=SEED, **kw)
    assert dec.rows == 9 + 12 - 1
    second = prompt[:, 2:7]
    t2 = dec.generate(second, 14, append=True, seed=SEED + 3, **kw)
    assert t2.shape == (batch, 19) and torch.equal(t2[:, :5], second)
    whole = torch.cat([t1, t2], dim=1)
    assert dec.rows == 39 and _counters(dec.cache) == [39, 39] and torch.equal(dec.s_hist[:, :40], whole)
    assert dec.spec_stats()[1] == 13
    _check_sampled(cycle_model, perm, whole, [(9, 12)], SEED, "turn 1", share=None)      # (a dozen columns: no share to speak of)
    _check_sampled(cycle_model, perm, whole, [(26, 14)], SEED + 3, "turn 2", share=None)


def test_refusals(cycle_model, decoders):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    with pytest.raises(ValueError, match="needs both"):
        GraphDecoder(cycle_model, 2, MAX_LEN, speculative=K, spec_sampling=True)                     # without sampling
    with pytest.raises(ValueError, match="needs both"):
        GraphDecoder(cycle_model, 2, MAX_LEN, sampling=True, spec_sampling=True)                     # without speculative
    with pytest.raises(ValueError, match="needs both"):
        GraphDecoder(cycle_model, 2, MAX_LEN, spec_sampling=True)
    with pytest.raises(ValueError, match="spec_sampling must be"):
        GraphDecoder(cycle_model, 2, MAX_LEN, speculative=K, sampling=True, spec_sampling=1)
    with pytest.raises(ValueError, match="greedy verification only"):                                # the pair without the flag
        GraphDecoder(cycle_model, 2, MAX_LEN, speculative=K, sampling=True)
    with pytest.raises(ValueError, match="ragged=True"):                                             # speculative's other requirements stay
        GraphDecoder(cycle_model, 2, MAX_LEN, speculative=K, sampling=True, spec_sampling=True, ragged=True)
    with pytest.raises(ValueError, match="fp16 cache rows"):
        GraphDecoder(cycle_model, 2, MAX_LEN, speculative=K, sampling=True, spec_sampling=True, kv_bits=8)
    # decoders built without the flag: no new attributes, the hand-over they always had
    for dec in (GraphDecoder(cycle_model, 2, MAX_LEN, capture=False), decoders(2, False, spec=False),
                GraphDecoder(cycle_model, 2, MAX_LEN, capture=False, speculative=K)):
        for name in ("spec_sampling", "s_spec_ws"):
            assert not hasattr(dec, name)
    spec = decoders(2, False)
    assert spec.spec_sampling is True and spec.s_spec_ws.shape == (2 * (K + 1),) and spec.s_spec_ws.dtype == torch.int64
