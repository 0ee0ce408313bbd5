"""``GraphDecoder(window=W, rolling=True)``: a sliding-window decoder on a ring cache.

The model is the tiny accelerated Llama of tests/test_gpu_window_decoder.py (hidden 256, 2 layers, vocab 512) at head sizes 64 (4
heads / 2 KV heads) and 128 (2 / 1).  Batch 2, W = 6, ``rolling_chunk=4``: the cache layers hold ring_rows(6, 4) = 128 rows.  A prompt
of 21 tokens (six pieces) and 150 new tokens make 171 positions, more than the ring: the steps run through the wrap.

Method and bound are that file's: the prompt's logits and every step's logits against the stock ``LlamaForCausalLM`` forward of the
whole generated sequence under a banded 4-D mask (key j for query i iff ``j <= i and j > i - W``), within 4e-3 * spread + 4e-3.
The captured and the eager rolling decoder agree in tokens and logits; a second turn (``append=True``) whose pieces cross the
ring's end stays within the bound; the cache tensors have 128 rows; no step is dropped.

Measured on an MI355X (the lines this file prints):
  prompt and 149 steps against the banded stock forward, worst share of the bound     0.137 (head 64)    0.182 (head 128)
  ... of them the steps whose new row has wrapped                                     0.130              0.127
  ... the same logits against the full causal forward (must exceed 1)                 235                222
  second turn across the ring's end against the banded stock forward                 0.00098 of 0.0092  0.00098 of 0.0086"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 256
B, P, NEW, W, CHUNK, R = 2, 21, 150, 6, 4, 128


def _tol(ref):
    return 4e-3 * ref.abs().max().item() + 4e-3


@pytest.fixture(scope="module", params=(64, 128), ids=("d64", "d128"))
def models(request):
    transformers = pytest.importorskip("transformers")
    from eetq_amd.utils import eet_accelerator
    heads, kv = (4, 2) if request.param == 64 else (2, 1)
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=heads,
                                   num_key_value_heads=kv, vocab_size=512, max_position_embeddings=512, attn_implementation="eager")
    torch.manual_seed(0)
    stock = transformers.LlamaForCausalLM(cfg).half().to(DEV).eval()
    model = eet_accelerator(copy.deepcopy(stock), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)
    return stock, model, cfg


@pytest.fixture(scope="module")
def prompt():
    g = torch.Generator().manual_seed(29)
    return torch.randint(1, 512, (B, P), generator=g).to(DEV)


def _decoder(model, **kw):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(model, B, MAX_LEN, window=W, rolling=True, rolling_chunk=CHUNK, **kw)


@pytest.fixture(scope="module")
def captured(models):
    return _decoder(models[1])


@pytest.fixture(scope="module")
def eager(models):
    return _decoder(models[1], capture=False)


@pytest.fixture(scope="module")
def reference_run(eager, prompt):
    """the eager rolling decoder on the prompt, computed once: (tokens, prompt logits, [step logits], dropped steps)"""
    import eetq_amd.ops as ops
    steps = []
    inner = eager._logits

    def recording():
        lg = inner()
        steps.append(lg.float().clone())
        return lg

    ops.decode_dropped_steps()
    eager._logits = recording
    try:
        tokens, first = eager.generate(prompt, NEW, return_prefill_logits=True)
    finally:
        del eager._logits
    return tokens.clone(), first.float().clone(), steps, ops.decode_dropped_steps()


def _banded_logits(model, tokens, window):
    """the stock forward of `model` on the whole sequence under the banded causal mask (no cache, no promise): [B, L, vocab] float"""
    L = tokens.shape[1]
    i, j = torch.arange(L, device=DEV)[:, None], torch.arange(L, device=DEV)[None, :]
    keep = (j <= i) & (j > i - window)
    mask = torch.zeros(L, L, dtype=torch.float16, device=DEV).masked_fill_(~keep, float("-inf"))
    with torch.no_grad():
        return model(tokens, attention_mask=mask[None, None].expand(tokens.shape[0], 1, L, L).contiguous(), use_cache=False).logits.float()


def _worst(ref, got_rows, first_col):
    return max((got - ref[:, first_col + i]).abs().max().item() / _tol(ref[:, first_col + i]) for i, got in enumerate(got_rows))


def _the_cache_is_a_ring_of_128_rows(captured, eager):
    from eetq_amd.utils.kv_cache import RollingStaticCache, ring_rows
    assert ring_rows(W, CHUNK) == R
    for dec in (captured, eager):
        assert isinstance(dec.cache, RollingStaticCache) and dec.rolling and dec.max_len == MAX_LEN
        for layer in dec.cache.layers:
            assert layer.keys.shape[2] == R and layer.values.shape[2] == R


def test_against_the_stock_model_under_a_banded_mask(models, prompt, reference_run):
    _, model, cfg = models
    tokens, first, steps, dropped = reference_run
    assert P + NEW > R, "the sequence is longer than the ring"
    assert tokens.shape == (B, P + NEW) and torch.equal(tokens[:, :P], prompt)
    assert len(steps) == NEW - 1 and all(torch.isfinite(x).all() for x in [first] + steps)
    assert dropped == 0, "a ring is never full: no step may be dropped"
    banded = _banded_logits(model, tokens[:, :-1], W)
    worst = _worst(banded, [first] + steps, P - 1)
    late = _worst(banded, steps[R - P:], R)      # the steps whose new row has wrapped
    causal = _worst(_banded_logits(model, tokens[:, :-1], 10 ** 6), [first] + steps, P - 1)
    print("rolling decoder vs the stock forward under the banded mask (head %d): worst |logits - stock| / bound = %.3f "
          "(steps behind the wrap: %.3f; against the full causal mask: %.3f)" % (cfg.head_dim or 0, worst, late, causal))
    assert worst < 1.0
    assert causal > 1.0, "the window changes these logits by more than the bound: the comparison above is not vacuous"


def test_captured_equals_eager(captured, eager, prompt, reference_run):
    import eetq_amd.ops as ops
    _the_cache_is_a_ring_of_128_rows(captured, eager)
    tokens, first = reference_run[:2]
    ops.decode_dropped_steps()
    got, lg = captured.generate(prompt, NEW, return_prefill_logits=True)
    assert ops.decode_dropped_steps() == 0
    assert torch.equal(got, tokens) and torch.equal(lg.float(), first)
    assert captured.rows == P + NEW - 1
    assert [int(l.cumulative_length) for l in captured.cache.layers] == [P + NEW - 1] * 2, "the counters count logical rows"


def test_sampling_decoder(models, prompt, reference_run):
    tokens = reference_run[0]
    dec = _decoder(models[1], sampling=True)
    assert torch.equal(dec.generate(prompt, NEW), tokens), "do_sample=False is the greedy decoder"
    kw = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=1234)
    a = dec.generate(prompt, NEW, **kw).clone()
    assert torch.equal(a, dec.generate(prompt, NEW, **kw)) and torch.equal(a[:, :P], prompt)


def test_second_turn_across_the_rings_end(models, captured, eager, prompt):
    import eetq_amd.ops as ops
    _, model, _ = models
    g = torch.Generator().manual_seed(9)
    more = torch.randint(1, 512, (B, 12), generator=g).to(DEV)
    ops.decode_dropped_steps()
    results = []
    for dec in (captured, eager):
        tokens = dec.generate(prompt, 100).clone()                # rows 0 .. 119 cached, one token pending
        assert dec.rows == P + 100 - 1 < R
        got, lg = dec.generate(more, 3, return_prefill_logits=True, append=True)    # 13 rows in pieces of 4: rows 120 .. 132
        rows = P + 100 + 12 + 3 - 1
        assert dec.rows == rows and [int(l.cumulative_length) for l in dec.cache.layers] == [rows] * 2
        assert got.shape == (B, 12 + 3) and torch.equal(got[:, :12], more)
        results.append((tokens, got.clone(), lg.float().clone()))
    assert ops.decode_dropped_steps() == 0
    assert all(torch.equal(a, b) for a, b in zip(*results)), "captured and eager agree across the wrap"
    tokens, _, lg = results[0]
    assert P + 100 - 1 < R < P + 100 + 12, "the second prompt's rows cross the ring's end"
    whole = torch.cat([tokens, more], 1)                       # every token the cache has seen when the second prompt ends
    want = _banded_logits(model, whole, W)[:, -1]
    err = (lg - want).abs().max().item()
    print("rolling decoder second turn across the ring's end: logits %.3g of %.3g" % (err, _tol(want)))
    assert err < _tol(want)


def test_refused_combinations(models):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    _, model, _ = models
    with pytest.raises(ValueError, match="rolling=True needs window"):
        GraphDecoder(model, B, MAX_LEN, rolling=True)
    with pytest.raises(ValueError, match="ragged"):
        GraphDecoder(model, B, MAX_LEN, window=W, rolling=True, ragged=True)
    with pytest.raises(ValueError, match="kv_bits"):
        GraphDecoder(model, B, MAX_LEN, window=W, rolling=True, kv_bits=8)
    with pytest.raises(ValueError, match="speculative"):
        GraphDecoder(model, B, MAX_LEN, window=W, rolling=True, speculative=3)
    with pytest.raises(ValueError, match="rolling_chunk"):
        GraphDecoder(model, B, MAX_LEN, window=W, rolling=True, rolling_chunk=0)
