"""``GraphDecoder(window=W)``: sliding-window attention through the prompt kernels and the captured decode graphs.

The model is the tiny accelerated Llama of tests/test_gpu_ragged_decoder.py (hidden 256, 2 layers, vocab 512) at head sizes 64 (4
heads / 2 KV heads) and 128 (2 / 1).  Batch 2, a prompt of 21 tokens, 8 new tokens, W = 6: every token from the seventh on has a
truncated window, in the prompt and in every step.

Against the stock path: the prompt's logits and every step's logits are compared with the stock ``LlamaForCausalLM`` forward of
the weights the decoder runs on, given a 4-D additive mask that keeps key j for query i iff ``j <= i and j > i - W`` (-inf
elsewhere), within the project's bound for this comparison, 4e-3 * spread + 4e-3.  Token equality with the stock model is not
asserted (near-ties may flip); it is asserted between the captured and the eager decoder.  A window that covers every length gives
the plain decoder's tokens and logits bit for bit.

Measured on an MI355X (the lines this file prints):
  prompt and seven steps against the banded stock forward, worst share of the bound   0.128 (head 64)    0.129 (head 128)
  ... the same logits against the full causal forward (must exceed 1)                 192                172
  prompt in pieces of 4 against the whole prompt, logits                              0.00073 of 0.0085  0.00098 of 0.0085
  second turn against the banded stock forward of the whole conversation              0.0010 of 0.0085   0.0012 of 0.0083"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 64
B, P, NEW, W = 2, 21, 8, 6


def _tol(ref):
    return 4e-3 * ref.abs().max().item() + 4e-3


@pytest.fixture(scope="module", params=(64, 128), ids=("d64", "d128"))
def models(request):
    transformers = pytest.importorskip("transformers")
    from eetq_amd.utils import eet_accelerator
    heads, kv = (4, 2) if request.param == 64 else (2, 1)
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=heads,
                                   num_key_value_heads=kv, vocab_size=512, max_position_embeddings=128, attn_implementation="eager")
    torch.manual_seed(0)
    stock = transformers.LlamaForCausalLM(cfg).half().to(DEV).eval()
    model = eet_accelerator(copy.deepcopy(stock), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)
    return stock, model, cfg


@pytest.fixture(scope="module")
def prompt():
    g = torch.Generator().manual_seed(29)
    return torch.randint(1, 512, (B, P), generator=g).to(DEV)


@pytest.fixture(scope="module")
def captured(models):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(models[1], B, MAX_LEN, window=W)


@pytest.fixture(scope="module")
def eager(models):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(models[1], B, MAX_LEN, capture=False, window=W)


@pytest.fixture(scope="module")
def reference_run(eager, prompt):
    """the eager windowed decoder on the prompt, computed once: (tokens, prompt logits, [step logits])"""
    steps = []
    inner = eager._logits

    def recording():
        lg = inner()
        steps.append(lg.float().clone())
        return lg

    eager._logits = recording
    try:
        tokens, first = eager.generate(prompt, NEW, return_prefill_logits=True)
    finally:
        del eager._logits
    return tokens.clone(), first.float().clone(), steps


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


def test_against_the_stock_model_under_a_banded_mask(models, prompt, reference_run):
    _, model, cfg = models
    tokens, first, steps = reference_run
    assert tokens.shape == (B, P + NEW) and torch.equal(tokens[:, :P], prompt)
    assert len(steps) == NEW - 1 and all(torch.isfinite(x).all() for x in [first] + steps)
    banded = _banded_logits(model, tokens[:, :-1], W)
    worst = _worst(banded, [first] + steps, P - 1)
    # the same comparison with the whole prefix attended: what a decoder that ignored the window would match
    causal = _worst(_banded_logits(model, tokens[:, :-1], 10 ** 6), [first] + steps, P - 1)
    print("windowed decoder vs the stock forward under the banded mask (head %d): worst |logits - stock| / bound = %.3f "
          "(against the full causal mask: %.3f)" % (cfg.head_dim or 0, worst, causal))
    assert worst < 1.0
    assert causal > 1.0, "the window changes these logits by more than the bound: the comparison above is not vacuous"


def test_captured_equals_eager(captured, prompt, reference_run):
    tokens, first, _ = reference_run
    got, lg = captured.generate(prompt, NEW, return_prefill_logits=True)
    assert torch.equal(got, tokens) and torch.equal(lg.float(), first)
    assert captured.rows == P + NEW - 1
    assert [int(l.cumulative_length) for l in captured.cache.layers] == [P + NEW - 1] * 2


def test_chunked_prompt(captured, eager, prompt, reference_run):
    first = reference_run[1]
    a, la = eager.generate(prompt, NEW, return_prefill_logits=True, prefill_chunk=4)
    b, lb = captured.generate(prompt, NEW, return_prefill_logits=True, prefill_chunk=4)
    assert torch.equal(a, b) and torch.equal(la, lb)
    err = (la.float() - first).abs().max().item()
    print("windowed decoder, prompt in pieces of 4: logits %.3g of %.3g" % (err, _tol(first)))
    assert err < _tol(first)


def test_a_window_over_every_length_is_the_plain_decoder(models, prompt):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    plain = GraphDecoder(models[1], B, MAX_LEN)
    want, wl = plain.generate(prompt, NEW, return_prefill_logits=True)
    wide = GraphDecoder(models[1], B, MAX_LEN, window=MAX_LEN)
    got, gl = wide.generate(prompt, NEW, return_prefill_logits=True)
    assert torch.equal(got, want) and torch.equal(gl, wl)


def test_sampling_decoder(models, prompt, reference_run):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    tokens = reference_run[0]
    dec = GraphDecoder(models[1], B, MAX_LEN, sampling=True, window=W)
    assert torch.equal(dec.generate(prompt, NEW), tokens), "do_sample=False is the greedy decoder"
    kw = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=1234)
    a = dec.generate(prompt, NEW, **kw).clone()
    assert torch.equal(a, dec.generate(prompt, NEW, **kw)) and torch.equal(a[:, :P], prompt)


def test_second_turn(models, captured, prompt, reference_run):
    _, model, _ = models
    tokens = reference_run[0]
    g = torch.Generator().manual_seed(9)
    more = torch.randint(1, 512, (B, 5), generator=g).to(DEV)
    assert torch.equal(captured.generate(prompt, NEW), tokens)
    got, lg = captured.generate(more, 3, return_prefill_logits=True, append=True)
    rows = P + NEW + 5 + 3 - 1
    assert captured.rows == rows and [int(l.cumulative_length) for l in captured.cache.layers] == [rows] * 2
    assert got.shape == (B, 5 + 3) and torch.equal(got[:, :5], more)
    whole = torch.cat([tokens, more], 1)                       # every token the cache has seen when the second prompt ends
    want = _banded_logits(model, whole, W)[:, -1]
    err = (lg.float() - want).abs().max().item()
    print("windowed decoder second turn: logits %.3g of %.3g" % (err, _tol(want)))
    assert err < _tol(want)


def test_refused_combinations(models):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    stock, model, _ = models
    with pytest.raises(ValueError, match="ragged=True"):
        GraphDecoder(model, B, MAX_LEN, window=W, ragged=True)
    with pytest.raises(ValueError, match="kv_bits"):
        GraphDecoder(model, B, MAX_LEN, window=W, kv_bits=8)
    with pytest.raises(ValueError, match="speculative"):
        GraphDecoder(model, B, MAX_LEN, window=W, speculative=3)
    with pytest.raises(ValueError, match="fully accelerated"):
        GraphDecoder(stock, B, MAX_LEN, window=W)
    with pytest.raises(ValueError, match="fully accelerated"):
        GraphDecoder(model, B, MAX_LEN, window=W, lean=False)
    with pytest.raises(ValueError, match="window must be"):
        GraphDecoder(model, B, MAX_LEN, window=0)
