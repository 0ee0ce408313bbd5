"""Prompts behind cached rows through the modules: ``appended_static_prefill`` against the stock attention path, and
``GraphDecoder`` with a chunked prompt (``prefill(chunk=)``, ``generate(prefill_chunk=)``) and a second turn
(``generate(append=True)``), greedy and sampling, captured and eager.

The model is the tiny accelerated Llama of tests/test_gpu_parity.py (hidden 256, 4 heads / 2 KV heads of 64, 2 layers, vocab 512).
Logits are compared within 4e-3 * spread + 4e-3, the tolerance test_eet_attention_static_cache_prompt_matches_stock_path uses for
the library's prompt kernel against the stock attention call.  Token equality between a two-turn run and a single fresh prompt is
deliberately not asserted: the projections take different kernel paths at different row counts, so a near-tie may flip."""
import contextlib
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 64


def _tol(ref):
    return 4e-3 * ref.abs().max().item() + 4e-3


@pytest.fixture(scope="module")
def cfg():
    transformers = pytest.importorskip("transformers")
    return transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4,
                                    num_key_value_heads=2, vocab_size=512, max_position_embeddings=128)


@pytest.fixture(scope="module")
def model(cfg):
    import transformers
    from eetq_amd.utils import eet_accelerator
    torch.manual_seed(0)
    stock = transformers.LlamaForCausalLM(cfg).half().to(DEV).eval()
    return eet_accelerator(copy.deepcopy(stock), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(11)
    return (torch.randint(0, 512, (2, 9), generator=g).to(DEV), torch.randint(0, 512, (2, 5), generator=g).to(DEV),
            torch.randint(0, 512, (2, 50), generator=g).to(DEV))


@pytest.fixture(scope="module")
def captured(model):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(model, 2, MAX_LEN)


@pytest.fixture(scope="module")
def eager(model):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return GraphDecoder(model, 2, MAX_LEN, capture=False)


def _counters(cache):
    return [int(layer.cumulative_length) for layer in cache.layers]


def test_appended_promise_against_the_stock_path(model, cfg):
    """24 tokens, then 13 more behind them: under the promise the appended chunk goes through ops.prefill_attention with the
    cache's counter as its device length, without it through the stock call under the model's mask.  Under the promise the rows
    at and beyond the counter are NaN: finite logits show that the library kernel ran, within its descriptor range."""
    import transformers
    import eetq_amd.modules.llama_modules as lm
    assert "appended_static_prefill" in lm.__all__
    g = torch.Generator().manual_seed(5)
    first, more = torch.randint(0, 512, (2, 24), generator=g).to(DEV), torch.randint(0, 512, (2, 13), generator=g).to(DEV)

    def run(promise):
        cache = transformers.StaticCache(config=cfg, max_cache_len=MAX_LEN)
        with torch.no_grad():
            model(first[:, :1], past_key_values=cache, use_cache=True)        # allocates the cache tensors
            cache.reset()
            a = model(first, past_key_values=cache, cache_position=torch.arange(24, device=DEV), use_cache=True).logits.float()
            assert _counters(cache) == [24, 24]
            if promise:
                for layer in cache.layers:
                    layer.keys[:, :, 24:] = float("nan")
                    layer.values[:, :, 24:] = float("nan")
            with (lm.appended_static_prefill() if promise else contextlib.nullcontext()):
                b = model(more, past_key_values=cache, cache_position=torch.arange(24, 37, device=DEV), use_cache=True).logits.float()
        return a, b, cache

    ra, rb, rc = run(False)
    pa, pb, pc = run(True)
    assert _counters(rc) == _counters(pc) == [37, 37]
    assert torch.equal(pc.layers[0].keys[:, :, :37], rc.layers[0].keys[:, :, :37])
    assert torch.equal(pc.layers[0].values[:, :, :37], rc.layers[0].values[:, :, :37])
    assert torch.isnan(pc.layers[1].keys[:, :, 37:]).all()
    assert torch.isfinite(pb).all() and torch.isfinite(rb).all()
    print("multiturn promise: |first| %.3g, |appended| %.3g of %.3g" % ((pa - ra).abs().max().item(), (pb - rb).abs().max().item(), _tol(rb)))
    assert (pa - ra).abs().max().item() < _tol(ra) and (pb - rb).abs().max().item() < _tol(rb)


@pytest.mark.parametrize("chunk", (7, 16, 64))
def test_chunked_prefill(eager, prompts, chunk):
    prompt = prompts[2]
    with torch.no_grad():
        ref = eager.prefill(prompt).logits[:, -1].float()
        layer = eager.cache.layers[0]
        rk, rv = layer.keys[:, :, :50].clone(), layer.values[:, :, :50].clone()
        assert _counters(eager.cache) == [50, 50] and eager.rows == 50
        for layer in eager.cache.layers:      # nothing may be left over from the unchunked call
            layer.keys.zero_()
            layer.values.zero_()
        got = eager.prefill(prompt, chunk=chunk).logits[:, -1].float()
    layer = eager.cache.layers[0]
    gk, gv = layer.keys[:, :, :50], layer.values[:, :, :50]
    assert _counters(eager.cache) == [50, 50] and eager.rows == 50
    if chunk >= 50:
        assert torch.equal(got, ref) and torch.equal(gk, rk) and torch.equal(gv, rv)
        return
    print("multiturn chunk %d: logits %.3g of %.3g, keys %.3g of %.3g" % (chunk, (got - ref).abs().max().item(), _tol(ref),
                                                                         (gk.float() - rk.float()).abs().max().item(), _tol(rk.float())))
    assert (gk.float() - rk.float()).abs().max().item() < _tol(rk.float())
    assert (gv.float() - rv.float()).abs().max().item() < _tol(rv.float())
    assert (got - ref).abs().max().item() < _tol(ref)


def _two_turns(dec, prompts, **kw):
    p1, p2 = prompts[0], prompts[1]
    t1 = dec.generate(p1, 6, **kw)
    assert dec.rows == 9 + 6 - 1
    t2, lg = dec.generate(p2, 6, append=True, return_prefill_logits=True, **kw)
    assert dec.rows == 9 + 6 + 5 + 6 - 1 and _counters(dec.cache) == [dec.rows] * 2
    assert t1.shape == (2, 15) and t2.shape == (2, 11) and torch.equal(t1[:, :9], p1) and torch.equal(t2[:, :5], p2)
    return t1, t2, lg.float()


def test_two_turns(captured, eager, prompts):
    t1, t2, lg = _two_turns(captured, prompts)
    # the second turn's prompt logits against a fresh decoder that is given the whole conversation as one prompt
    whole = torch.cat([t1, prompts[1]], dim=1)
    with torch.no_grad():
        ref = eager.prefill(whole).logits[:, -1].float()
    print("multiturn two turns: prompt logits %.3g of %.3g" % ((lg - ref).abs().max().item(), _tol(ref)))
    assert (lg - ref).abs().max().item() < _tol(ref)
    e1, e2, _ = _two_turns(eager, prompts)
    assert torch.equal(e1, t1) and torch.equal(e2, t2)
    r1, r2, _ = _two_turns(captured, prompts)          # the first generate is a fresh one: the conversation starts over
    assert torch.equal(r1, t1) and torch.equal(r2, t2)


def test_two_turns_on_a_sampling_decoder(model, captured, prompts):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    t1, t2, _ = _two_turns(captured, prompts)
    dec = GraphDecoder(model, 2, MAX_LEN, sampling=True)
    s1, s2, _ = _two_turns(dec, prompts, do_sample=False)
    assert torch.equal(s1, t1) and torch.equal(s2, t2)
    a1, a2, _ = _two_turns(dec, prompts, do_sample=True, seed=3)
    b1, b2, _ = _two_turns(dec, prompts, do_sample=True, seed=3)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)


def test_refusals_and_edge_uses(model, captured, eager, prompts):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    p1 = prompts[0]
    captured.generate(p1, 6)
    with pytest.raises(ValueError):
        captured.generate(prompts[2], 6, append=True)             # 14 + 1 + 50 + 6 rows > 64
    captured.prefill(prompts[2][:, :40], append=True)             # 14 + 40 rows
    assert captured.rows == 54 and _counters(captured.cache) == [54, 54]
    with pytest.raises(ValueError):
        captured.prefill(prompts[2][:, :11], append=True)
    empty = GraphDecoder(model, 2, MAX_LEN, capture=False)
    assert empty.rows == 0
    a = empty.generate(p1, 6, append=True)                        # nothing cached: a plain generate
    assert empty.rows == 14 and torch.equal(a, eager.generate(p1, 6))
    c = captured.generate(prompts[2][:, :21], 6, prefill_chunk=4)
    e = eager.generate(prompts[2][:, :21], 6, prefill_chunk=4)
    plain = eager.generate(prompts[2][:, :21], 6)
    assert c.shape == plain.shape == (2, 27) and torch.equal(c, e)
