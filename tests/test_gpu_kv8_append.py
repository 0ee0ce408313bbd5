"""``GraphDecoder(..., kv_bits=8, kv8_append=True)``: multi-turn and chunked prompts on the int8 KV cache, on the two tiny
accelerated Llamas of tests/test_gpu_kv8_decoder.py (2 KV heads of 64 with 64 cache rows; 1 KV head of 128 with 200 rows), batch 2.

A piece behind cached rows writes its rows first (rotated, quantised, behind the device counter) and then attends the dequantised
rows below the advanced counter through ops.prefill_attention_i8kv.  Asserted: the captured and the eager decoder emit the same
tokens and leave the same int8 bytes and scale bits in every layer, with the counters (and ``dec.rows``) at the expected row;
layer 0's appended rows are the NumPy quantiser of the fp16 decoder's layer-0 rows (they do not depend on attention); the block's
attention output for 5 tokens appended behind 12 is within 2e-3 of torch float32 attention over the dequantised cache (the
project's bound for the decode step, test_gpu_kv8_decoder._decode_step_attention_against_float32); ``prefill_chunk >= P`` is the
fresh path and gives the fp16 decoder's logits bit for bit.  NOT asserted, printed for DESIGN.md 4.7: the largest logit
difference of a chunked int8 prompt against the whole int8 prompt and against the fp16 decoder (there is no reference figure; it
must be finite)."""
import numpy as np
import pytest
import torch

import kv8_cases as k8c
from test_gpu_kv8_decoder import (MAX_LEN, MAX_LEN_128, _filled_rows, _same_rows, cfg, cfg128, model, model128, prompt,  # noqa: F401
                                  stock)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NEW = 6


@pytest.fixture(scope="module")
def more():
    return torch.randint(0, 512, (2, 7), generator=torch.Generator().manual_seed(12)).to(DEV)


def _decoders(model, max_len):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    return (GraphDecoder(model, 2, max_len, kv_bits=8, kv8_append=True),
            GraphDecoder(model, 2, max_len, capture=False, kv_bits=8, kv8_append=True))


@pytest.fixture(scope="module")
def pair(model):
    return _decoders(model, MAX_LEN)


@pytest.fixture(scope="module")
def pair128(model128):
    return _decoders(model128, MAX_LEN_128)


def _two_turns_and_chunks(pair, prompt, more):
    dec, eager = pair
    P, M = prompt.shape[1], more.shape[1]
    rows1 = P + N_NEW - 1
    rows2 = rows1 + 1 + M + N_NEW - 1          # the pending token, the second prompt, this turn's tokens but the last
    outs = []
    for d in (dec, eager):
        first = d.generate(prompt, N_NEW)
        assert d.rows == rows1 and [int(l.cumulative_length) for l in d.cache.layers] == [rows1] * len(d.cache.layers)
        second = d.generate(more, N_NEW, append=True)
        assert first.shape == (2, P + N_NEW) and second.shape == (2, M + N_NEW) and torch.equal(second[:, :M], more)
        assert d.rows == rows2
        outs.append((first, second, _filled_rows(d, rows2)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "captured against eager: tokens"
    _same_rows(outs[0][2], outs[1][2], "two turns, captured against eager")
    # a chunked prompt: pieces of 4, 4 and 1 token (the last one is a decode step behind the counter)
    outs = []
    for d in (dec, eager):
        toks = d.generate(prompt, N_NEW, prefill_chunk=4)
        assert d.rows == rows1
        outs.append((toks, _filled_rows(d, rows1)))
    assert torch.equal(outs[0][0], outs[1][0]), "captured against eager: tokens of the chunked prompt"
    _same_rows(outs[0][1], outs[1][1], "chunked prompt, captured against eager")


def test_two_turns_and_chunked_prompt(pair, prompt, more):
    _two_turns_and_chunks(pair, prompt, more)


def test_two_turns_and_chunked_prompt_head_size_128(pair128, prompt, more):
    _two_turns_and_chunks(pair128, prompt, more)


def _layer0_rows(model, pair, max_len, prompt, more):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    fp16 = GraphDecoder(model, 2, max_len, capture=False)
    dec = pair[1]
    P, M = prompt.shape[1], more.shape[1]
    for d in (fp16, dec):
        d.prefill(prompt)
        d.prefill(more, append=True)
        assert d.rows == P + M
    l16, l8 = fp16.cache.layers[0], dec.cache.layers[0]
    assert int(l8.cumulative_length) == int(l16.cumulative_length) == P + M
    ek8, eks = k8c.quantize_rows(l16.keys[:, :, : P + M].cpu().numpy())
    ev8, evs = k8c.quantize_rows(l16.values[:, :, : P + M].cpu().numpy())
    assert np.array_equal(l8.keys[:, :, : P + M].cpu().numpy(), ek8) and np.array_equal(l8.values[:, :, : P + M].cpu().numpy(), ev8)
    assert np.array_equal(l8.scales[:, :, : P + M].cpu().numpy().view(np.int16), k8c.scale_pairs(eks, evs).view(np.int16))


def test_layer0_appended_rows_are_the_quantised_fp16_rows(model, pair, prompt, more):
    _layer0_rows(model, pair, MAX_LEN, prompt, more)


def test_layer0_appended_rows_are_the_quantised_fp16_rows_head_size_128(model128, pair128, prompt, more):
    _layer0_rows(model128, pair128, MAX_LEN_128, prompt, more)


def _appended_attention_against_float32(model, cfg, max_len):
    from eetq_amd.utils.kv_cache import Int8StaticCache
    import eetq_amd.modules.llama_modules as lm
    attn = model.model.layers[0].self_attn
    h, hkv, d = attn.num_heads, attn.num_key_value_heads, attn.head_dim
    cache = Int8StaticCache(cfg, max_len).allocate(2, DEV)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 12, 256, generator=g) * 0.5).half().to(DEV)
    x5 = (torch.randn(2, 5, 256, generator=g) * 0.5).half().to(DEV)
    seen = {}
    hook = attn.o_proj.register_forward_pre_hook(lambda mod, args: seen.__setitem__("attn", args[0].clone()))
    try:
        with torch.no_grad(), lm.fresh_static_prefill():
            attn(x, past_key_values=cache, position_ids=torch.arange(12, device=DEV)[None].expand(2, 12))
        with torch.no_grad():
            qkv = attn.qkv_proj(x5)
            with lm.appended_static_prefill(), pytest.raises(NotImplementedError, match="int8 K and V"):      # without the opt-in
                attn(x5, past_key_values=cache, position_ids=torch.arange(12, 17, device=DEV)[None].expand(2, 5))
            assert int(cache.layers[0].cumulative_length) == 12
            with lm.appended_static_prefill(int8_rows=True):
                attn(x5, past_key_values=cache, position_ids=torch.arange(12, 17, device=DEV)[None].expand(2, 5))
    finally:
        hook.remove()
    layer = cache.layers[0]
    assert int(layer.cumulative_length) == 17
    q = qkv[..., : h * d].unflatten(-1, (h, d)).clone()                           # [2, 5, h, d]
    k_unused = torch.zeros(2, hkv, d, dtype=torch.float16, device=DEV)
    for t in range(5):
        qt = q[:, t].contiguous()
        attn.rotary_emb(qt, k_unused, torch.full((2,), 12 + t, dtype=torch.int64, device=DEV))
        q[:, t] = qt
    kd = (layer.keys[:, :, :17].float() * layer.scales[:, :, :17, 0:1].float()).repeat_interleave(h // hkv, dim=1)
    vd = (layer.values[:, :, :17].float() * layer.scales[:, :, :17, 1:2].float()).repeat_interleave(h // hkv, dim=1)
    s = torch.einsum("bthd,bhsd->bhts", q.float(), kd) * attn.scaling
    allowed = torch.arange(17, device=DEV)[None, :] <= (torch.arange(5, device=DEV)[:, None] + 12)
    p = torch.softmax(s.masked_fill(~allowed, float("-inf")), dim=-1)
    ref = torch.einsum("bhts,bhsd->bthd", p, vd).reshape(2, 5, h * d)
    err = (seen["attn"].float() - ref).abs().max().item()
    print("kv8 append: 5 tokens behind 12 (head size %d) against float32 over the dequantised cache: %.3e" % (d, err))
    assert seen["attn"].shape == ref.shape and torch.isfinite(seen["attn"]).all() and err < 2e-3


def test_appended_attention_against_float32(model, cfg):
    _appended_attention_against_float32(model, cfg, MAX_LEN)


def test_appended_attention_against_float32_head_size_128(model128, cfg128):
    _appended_attention_against_float32(model128, cfg128, MAX_LEN_128)


def _chunk_figures(model, pair, max_len, prompt):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    fp16 = GraphDecoder(model, 2, max_len, capture=False)
    dec = pair[1]
    P = prompt.shape[1]
    _, ref16 = fp16.generate(prompt, 1, return_prefill_logits=True)
    _, whole = dec.generate(prompt, 1, return_prefill_logits=True)
    # prefill_chunk >= P: one piece, on the fresh path -- the fp16 decoder's bits
    for chunk in (P, P + 5):
        _, one = dec.generate(prompt, 1, return_prefill_logits=True, prefill_chunk=chunk)
        assert torch.equal(one.view(torch.int16), ref16.view(torch.int16)), chunk
    assert torch.equal(whole.view(torch.int16), ref16.view(torch.int16))
    for chunk in (5, 2):
        _, part = dec.generate(prompt, 1, return_prefill_logits=True, prefill_chunk=chunk)
        assert torch.isfinite(part).all() and dec.rows == P
        print("kv8 append (head size %d): prompt of %d in pieces of %d: largest |logit - whole int8 prompt| %.4f, |logit - fp16 decoder| "
              "%.4f (largest |logit| %.3f)" % (model.model.layers[0].self_attn.head_dim, P, chunk, (part.float() - whole.float()).abs().max().item(),
                                              (part.float() - ref16.float()).abs().max().item(), ref16.float().abs().max().item()))


def test_one_piece_is_the_fresh_path_and_chunk_figures(model, pair, prompt):
    _chunk_figures(model, pair, MAX_LEN, prompt)


def test_one_piece_is_the_fresh_path_and_chunk_figures_head_size_128(model128, pair128, prompt):
    _chunk_figures(model128, pair128, MAX_LEN_128, prompt)


def test_argument_validation(model, prompt):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    with pytest.raises(ValueError, match="kv8_append"):
        GraphDecoder(model, 2, MAX_LEN, kv_bits=16, kv8_append=True)
    with pytest.raises(ValueError, match="kv8_append"):
        GraphDecoder(model, 2, MAX_LEN, kv8_append=True)
    plain = GraphDecoder(model, 2, MAX_LEN, capture=False, kv_bits=8)
    assert plain.kv8_append is False
    with pytest.raises(ValueError, match="int8 cache.*kv8_append=True"):          # the default decoder raises as before, naming the switch
        plain.generate(prompt, 2, append=True)
    with pytest.raises(ValueError, match="int8 cache.*kv8_append=True"):
        plain.prefill(prompt, chunk=4)


def test_no_state_is_left_on_the_model(model, pair, prompt):
    """A default int8 decoder on the SAME model still refuses after an opted-in decoder has appended, and the promise flags are
    down."""
    import eetq_amd.modules.llama_modules as lm
    from eetq_amd.utils.graph_decoder import GraphDecoder
    pair[1].generate(prompt, 2)
    pair[1].generate(prompt, 2, append=True)
    p = lm._prefill_promise
    assert not getattr(p, "int8_rows", False) and not getattr(p, "appended", False) and not getattr(p, "fresh", False)
    plain = GraphDecoder(model, 2, MAX_LEN, capture=False, kv_bits=8)
    plain.generate(prompt, 2)
    ids = torch.arange(5, device=DEV)
    with torch.no_grad(), lm.appended_static_prefill(), pytest.raises(NotImplementedError, match="int8 K and V"):
        model(prompt[:, :5], past_key_values=plain.cache, cache_position=ids, use_cache=True)
