"""``GraphDecoder(speculative=k, kv_bits=8, kv8_append=True, spec_attention="prompt" | "rows")``: speculative decoding on the int8 KV
cache, on the tiny accelerated Llama of tests/test_gpu_spec_decoder.py (hidden 256, 4 heads / 2 KV heads of 64, 2 layers, vocab 512),
96 cache rows, k = 4 -- its models, its orbit, its counters and its tolerance, imported from there -- and, for one test, the
head-128 / one-kv-head model of tests/test_gpu_kv8_decoder.py.  The verify step writes its k + 1 rows quantised behind the device
counter and attends the DEQUANTISED rows: through ``ops.prefill_attention_i8kv`` ("prompt") or ``ops.decode_attention_rows_i8kv``
("rows", the few-row kernel's int8 form).

The random model's tokens are judged against teacher-forced logits of the PLAIN int8 decoder: its eager one-token steps over the
finished sequence, the VALU decode kernel on int8 rows, none of the code under test.  Criterion, as in the fp16 files: rowmax -
logit[token] <= 2 (4e-3 max|logits| + 4e-3).  Measured on an MI355X (40 tokens, batch 2, lookup drafts, 29 verify steps for 39
tokens in either mode), worst gap of the criterion's 0.0179: "rows" 0, "prompt" 0 -- every emitted token IS the plain int8
decoder's argmax, and both modes meet the criterion itself.  (Had "prompt", whose kernel was merged before this file, exceeded it,
the excess would come from quantised rows that flip -- a cache row written from a slightly different hidden state can round to
other bytes -- and "rows" would be held to twice the "prompt" figure instead; the test says so in code, and it did not happen.)
One verify step's logits from identical cache bytes, "rows" against "prompt": 0.00098 of 0.0162 (4 / 2 heads of 64), 0.00049 of
0.0167 (2 / 1 heads of 128).  21 cases, 8.2 s wall for the file, 5.2 s of it the module's first model and its eight cycle decoders.

On the compiled boundary a missing ``ops.decode_attention_rows_i8kv`` FAILS these tests; only the ctypes boundary skips."""
import pytest
import torch

import test_gpu_spec_decoder as base
from test_gpu_kv8_decoder import cfg128, model128  # noqa: F401  (fixtures)
from test_gpu_spec_decoder import cfg, cycle_model, model, perm, prompts, stock  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = base.DEV
MAX_LEN, K, VOCAB = base.MAX_LEN, base.K, base.VOCAB
assert (MAX_LEN, K) == (96, 4)
MODES = ("rows", "prompt")
INT8_OPS = {"rows": "decode_attention_rows_i8kv", "prompt": "prefill_attention_i8kv"}


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.BOUNDARY != "ext":
        pytest.skip("decode_attention_rows_i8kv lives in the compiled module")
    assert o.decode_attention_rows_i8kv is not None, "the compiled module lacks decode_attention_rows_i8kv"
    return o


def _decoder(model, batch, capture=True, mode="rows", **kw):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(model, batch, MAX_LEN, capture=capture, speculative=K, kv_bits=8, kv8_append=True, spec_attention=mode, **kw)


def _plain8(model, batch=2, **kw):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(model, batch, MAX_LEN, kv_bits=8, **kw)


@pytest.fixture(scope="module")
def cycle_decoders(ops, cycle_model):
    return {(m, b, cap): _decoder(cycle_model, b, capture=cap, mode=m) for m in MODES for b in (1, 2) for cap in (True, False)}


@pytest.mark.parametrize("capture", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_cycle_model_tokens_and_accepted_drafts(cycle_decoders, perm, mode, batch, capture):
    dec = cycle_decoders[(mode, batch, capture)]
    assert dec.spec_attention == mode and dec.kv_bits == 8 and (dec.graph_spec is not None) == capture
    assert type(dec.cache.layers[0]).__name__ == "Int8StaticLayer" and dec.cache.layers[0].keys.dtype == torch.int8
    rows = [[first] + base._orbit(perm, first, 8) for first in (10, 23)[:batch]]
    prompt = torch.tensor(rows, device=DEV)
    for new in (1, 2, 5, 6, 23):
        got = dec.generate(prompt, new)
        want = [r + base._orbit(perm, r[-1], new) for r in rows]
        assert got.tolist() == want, (new, got.tolist(), want)
        steps, tokens = dec.spec_stats()
        assert tokens == new - 1 and steps <= -(-new // (K + 1)) + 2, (new, steps, tokens)
        assert dec.rows == 9 + new - 1 and base._counters(dec.cache) == [dec.rows] * 2 and int(dec.s_pos) == dec.rows
        assert dec.s_hist[:, :9 + new].tolist() == want and int(dec.s_tok[0, 0]) == want[0][-1]
    assert dec.spec_stats() == (5, 22), "23 tokens in ceil(22 / 5) = 5 verify steps"


def _ready_for_one_step(dec, prompt):
    """the state generate(prompt, K + 2) has before its first verify step (the fresh prompt runs on the fp16 prompt kernel)"""
    dec.generate(prompt, 1)
    dec.s_limit.fill_(K + 2)


ATTENTION_OPS = ("decode_attention_rows_i8kv", "prefill_attention_i8kv", "prefill_attention", "decode_attention_rows")


def _count_calls(monkeypatch, ops):
    calls = dict.fromkeys(ATTENTION_OPS, 0)
    for name in ATTENTION_OPS:
        def counted(*a, _name=name, _op=getattr(ops, name), **kw):
            calls[_name] += 1
            return _op(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    return calls


@pytest.mark.parametrize("mode", MODES)
def test_the_kernel_is_actually_used(ops, model, prompts, monkeypatch, mode):
    """one eager verify step: once per layer through the chosen int8 operator, never through the other one or an fp16 one"""
    dec = _decoder(model, 2, capture=False, mode=mode)
    _ready_for_one_step(dec, prompts[0])
    calls = _count_calls(monkeypatch, ops)
    dec._advance_spec()
    want = dict.fromkeys(ATTENTION_OPS, 0)
    want[INT8_OPS[mode]] = len(model.model.layers)
    assert calls == want, calls


def _one_step_logits(model, dec, prompt):
    _ready_for_one_step(dec, prompt)
    seen = []
    hook = model.lm_head.register_forward_hook(lambda mod, args, out, _seen=seen: _seen.append(out.float().clone()))
    try:
        dec._advance_spec()
    finally:
        hook.remove()
    assert len(seen) == 1 and seen[0].shape == (prompt.shape[0], K + 1, VOCAB)
    return seen[0]


def _rows_against_prompt(model, prompt, what):
    got = {mode: _one_step_logits(model, _decoder(model, 2, capture=False, mode=mode), prompt) for mode in MODES}
    tol = 2 * base._tol(got["prompt"])
    worst = (got["rows"] - got["prompt"]).abs().max().item()
    print("spec kv8 decoder %s: verify-step logits, rows against prompt: %.3g of %.3g" % (what, worst, tol))
    assert worst <= tol and not torch.isnan(got["rows"]).any() and not torch.isnan(got["prompt"]).any()


def test_logits_agree_with_the_prompt_kernel(ops, model, prompts):
    """one eager verify step from the same cache state (identical bytes) under "rows" and under "prompt": one function, two tilings"""
    _rows_against_prompt(model, prompts[0], "heads 4 / 2 x 64")


def test_logits_agree_with_the_prompt_kernel_head_size_128(ops, model128, prompts):
    assert model128.model.layers[0].self_attn.head_dim == 128
    _rows_against_prompt(model128, prompts[0], "heads 2 / 1 x 128")
    dec = _decoder(model128, 2)
    seq = dec.generate(prompts[0], 12)
    assert seq.shape == (2, 21) and dec.rows == 20 and base._counters(dec.cache) == [20, 20] and torch.equal(dec.s_hist[:, :21], seq)


@pytest.mark.parametrize("mode", MODES)
def test_unread_rows_do_not_matter(ops, model, prompts, mode):
    """every byte 0x80 and every scale NaN before generate: the rows a token attends were written first, the others are never read"""
    out = []
    for poison in (False, True):
        dec = _decoder(model, 2, capture=False, mode=mode)
        if poison:
            for layer in dec.cache.layers:
                layer.keys.fill_(-128)
                layer.values.fill_(-128)
                layer.scales.fill_(float("nan"))
        seen = []
        hook = model.lm_head.register_forward_hook(lambda mod, args, o, _seen=seen: _seen.append(o.clone()))
        try:
            seq = dec.generate(prompts[0], 20)
        finally:
            hook.remove()
        assert not torch.isnan(seen[-1]).any() and seen[-1].shape[1] == K + 1, "the final step is a verify step"
        out.append((seq, seen[-1], dec.spec_stats()))
    assert torch.equal(out[0][0], out[1][0]) and out[0][2] == out[1][2]
    assert torch.equal(out[0][1].view(torch.int16), out[1][1].view(torch.int16)), "the final step's logits, bit for bit"


def _teacher_forced_gap(plain, seq, first):
    """worst rowmax - logit[token] over the emitted columns first .. S - 1, against the plain int8 decoder's own logits: its prompt
    pass for column `first`, then one eager decode step per fed token (its cache rows come from ITS hidden states)"""
    S = seq.shape[1]
    with torch.no_grad():
        logits = [plain.prefill(seq[:, :first]).logits[:, -1].float().clone()]
        for c in range(first, S - 1):
            plain.s_tok.copy_(seq[:, c:c + 1])
            plain.s_pos.fill_(c)
            logits.append(plain._logits().float().clone())
    assert base._counters(plain.cache) == [S - 1] * 2
    logits = torch.stack(logits, dim=1)                                            # [B, S - first, V]: entry i predicts column first + i
    gap = logits.max(-1).values - logits.gather(2, seq[:, first:, None])[..., 0]
    assert not torch.isnan(logits).any()
    return gap.max().item(), 2 * base._tol(logits)


def test_random_model_every_token_is_an_argmax_of_the_plain_int8_decoder(ops, model, prompts):
    plain = _plain8(model, capture=False)
    worst = {}
    for mode in MODES:
        dec = _decoder(model, 2, mode=mode)
        seq = dec.generate(prompts[0], 40)
        steps, tokens = dec.spec_stats()
        assert tokens == 39 and 8 <= steps <= 39 and dec.rows == 48 and base._counters(dec.cache) == [48, 48]
        assert torch.equal(dec.s_hist[:, :49], seq)
        worst[mode], tol = _teacher_forced_gap(plain, seq, 9)
        print("spec kv8 decoder %s: lookup drafts, %d steps for 39 tokens, worst rowmax - logit[token] %.3g of %.3g"
              % (mode, steps, worst[mode], tol))
    if worst["prompt"] <= tol:
        assert worst["rows"] <= tol, worst
    else:   # quantised-row flips already move the merged route past the criterion: "rows" may not be worse than twice that
        assert worst["rows"] <= 2 * worst["prompt"], worst


@pytest.mark.parametrize("mode", MODES)
def test_sampled_verification(ops, cycle_model, cycle_decoders, perm, mode):
    """spec_sampling=True verification on the int8 cache: at temperature 0 it is the greedy int8 speculative decoder; a seed reproduces"""
    dec = _decoder(cycle_model, 2, mode=mode, sampling=True, spec_sampling=True)
    rows = [[first] + base._orbit(perm, first, 8) for first in (10, 23)]
    prompt = torch.tensor(rows, device=DEV)
    greedy = cycle_decoders[(mode, 2, True)].generate(prompt, 23)
    assert torch.equal(dec.generate(prompt, 23, do_sample=True, temperature=0.0, seed=5), greedy)
    assert dec.spec_stats() == (5, 22)
    assert torch.equal(dec.generate(prompt, 23), greedy)                             # do_sample=False
    drawn = dec.generate(prompt, 23, do_sample=True, temperature=0.6, seed=5)
    assert drawn.shape == (2, 32) and torch.equal(drawn, dec.generate(prompt, 23, do_sample=True, temperature=0.6, seed=5))


@pytest.fixture(scope="module")
def spec8(ops, model):
    return _decoder(model, 2)


def test_two_turns(spec8, prompts):
    """a second turn behind a speculative one: the pending token and the prompt go behind the cached int8 rows, the history follows"""
    t1 = spec8.generate(prompts[0], 12)
    assert t1.shape == (2, 21) and spec8.rows == 9 + 12 - 1
    t2 = spec8.generate(prompts[1], 14, append=True)
    assert t2.shape == (2, 19) and torch.equal(t2[:, :5], prompts[1])
    whole = torch.cat([t1, t2], dim=1)
    assert spec8.rows == 39 and base._counters(spec8.cache) == [39, 39] and int(spec8.s_pos) == 39
    assert torch.equal(spec8.s_hist[:, :40], whole) and spec8.spec_stats()[1] == 13


def test_chunked_prompt_and_the_plain_graphs(spec8, model, prompts):
    """prefill_chunk= and speculate=False work as on any kv8_append decoder: the plain graphs are the plain int8 decoder's"""
    plain = _plain8(model, kv8_append=True)
    a = spec8.generate(prompts[0], 20, speculate=False)
    assert torch.equal(a, plain.generate(prompts[0], 20)) and spec8.spec_stats() == (0, 0)
    assert torch.equal(spec8.s_hist[:, :29], a) and spec8.rows == 28 and base._counters(spec8.cache) == [28, 28]
    c = spec8.generate(prompts[0], 10, prefill_chunk=4)
    assert c.shape == (2, 19) and spec8.rows == 18 and base._counters(spec8.cache) == [18, 18] and spec8.spec_stats()[1] == 9
    assert torch.equal(spec8.s_hist[:, :19], c)


def test_refusals(ops, model, monkeypatch):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    with pytest.raises(ValueError, match="fp16 cache rows"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, kv_bits=8)
    with pytest.raises(ValueError, match="fp16 cache rows"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, kv_bits=8, spec_attention="rows")
    with pytest.raises(ValueError, match="kv8_append"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, kv_bits=16, kv8_append=True)
    with pytest.raises(ValueError, match="ragged=True"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, kv_bits=8, kv8_append=True, ragged=True)
    monkeypatch.setattr(ops, "decode_attention_rows_i8kv", None)
    with pytest.raises(ValueError, match="compiled operator module"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, kv_bits=8, kv8_append=True, spec_attention="rows")
    assert GraphDecoder(model, 2, MAX_LEN, capture=False, speculative=K, kv_bits=8, kv8_append=True).spec_attention == "prompt"


def test_defaults_are_unchanged(ops, model, prompts):
    """an fp16 speculative decoder and a plain kv_bits=8 decoder produce the same tokens built alone and built next to an int8
    speculative decoder of the same model"""
    from eetq_amd.utils.graph_decoder import GraphDecoder
    spec16, plain8 = GraphDecoder(model, 2, MAX_LEN, speculative=K), _plain8(model)
    assert spec16.kv_bits == 16 and spec16.spec_attention == "prompt" and plain8.speculative == 0 and plain8.graph_spec is None
    before16, stats = spec16.generate(prompts[0], 30), spec16.spec_stats()
    before8 = plain8.generate(prompts[0], 30)
    for mode in MODES:
        _decoder(model, 2, mode=mode).generate(prompts[0], 30)
    assert torch.equal(spec16.generate(prompts[0], 30), before16) and spec16.spec_stats() == stats
    assert torch.equal(plain8.generate(prompts[0], 30), before8)
    assert torch.equal(GraphDecoder(model, 2, MAX_LEN, speculative=K).generate(prompts[0], 30), before16)
    assert torch.equal(_plain8(model).generate(prompts[0], 30), before8)
