"""``GraphDecoder(..., kv_dtype="fp8_e4m3")``: the fp8 KV cache through the modules, on the two tiny accelerated Llamas of
tests/test_gpu_kv8_decoder.py (4 heads / 2 KV heads of 64 with 64 cache rows; 2 heads / 1 KV head of 128 with 200 rows, where the
decode step's default is more than one chunk)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIGS = {64: dict(heads=4, kv_heads=2, max_len=64, steps=20, seed=0), 128: dict(heads=2, kv_heads=1, max_len=200, steps=40, seed=1)}
SCALES = (0.5, 2.0)


def quant(x, s):
    return (x.cpu().float() / s).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _setup(head_dim):
    import transformers
    from eetq_amd.utils import eet_accelerator
    from eetq_amd.utils.graph_decoder import GraphDecoder
    c = CONFIGS[head_dim]
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=c["heads"],
                                   num_key_value_heads=c["kv_heads"], vocab_size=512, max_position_embeddings=256)
    torch.manual_seed(c["seed"])
    stock = transformers.LlamaForCausalLM(cfg).half().to(DEV).eval()
    model = eet_accelerator(copy.deepcopy(stock), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)
    assert model.model.layers[0].self_attn.head_dim == head_dim
    prompt = torch.randint(0, 512, (2, 9), generator=torch.Generator().manual_seed(11)).to(DEV)
    return dict(c, stock=stock, model=model, prompt=prompt, fp16=GraphDecoder(model, 2, c["max_len"]),
                fp8=GraphDecoder(model, 2, c["max_len"], kv_dtype="fp8_e4m3"))


def _prompt_logits_cache_rows_and_set_scales(setup):
    """Prompt logits equal the fp16 decoder's bit for bit at either scale pair; every layer's bytes below the counter are the
    torch quantiser of the fp16 decoder's rows, under the default scales and under ``set_scales``; ``reset`` keeps the scales."""
    from eetq_amd.utils.kv_cache import Fp8StaticCache
    fp16, fp8, prompt, P = setup["fp16"], setup["fp8"], setup["prompt"], setup["prompt"].shape[1]
    assert isinstance(fp8.cache, Fp8StaticCache)
    a = fp16.prefill(prompt).logits
    try:
        for ks, vs in ((1.0, 1.0), SCALES):
            fp8.cache.set_scales(ks, vs)
            fp8.cache.reset()
            assert all(torch.equal(l.scales.cpu(), torch.tensor([[ks, vs]] * l.scales.shape[0])) for l in fp8.cache.layers)
            b = fp8.prefill(prompt).logits
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
            for l16, l8 in zip(fp16.cache.layers, fp8.cache.layers):
                assert int(l8.cumulative_length) == int(l16.cumulative_length) == P and l8.keys.dtype == torch.float8_e4m3fn
                assert torch.equal(l8.keys[:, :, :P].cpu().view(torch.uint8), quant(l16.keys[:, :, :P], ks))
                assert torch.equal(l8.values[:, :, :P].cpu().view(torch.uint8), quant(l16.values[:, :, :P], vs))
        with pytest.raises(ValueError, match="positive and finite"):
            fp8.cache.set_scales(0.0, 1.0)
        with pytest.raises(ValueError, match="per kv head"):
            fp8.cache.set_scales(torch.ones(7), 1.0)
    finally:
        fp8.cache.set_scales(1.0, 1.0)


def _filled(decoder, rows):
    assert [int(l.cumulative_length) for l in decoder.cache.layers] == [rows] * 2
    return [torch.stack([l.keys[:, :, :rows].view(torch.uint8), l.values[:, :, :rows].view(torch.uint8)]).clone()
            for l in decoder.cache.layers]


def _captured_eager_and_unfused_steps(setup):
    """The captured one-launch step (replayed many times), the same step launched eagerly and the unfused step (write launch +
    two-launch attention) emit the same tokens and leave the same cache bytes behind; at head size 128 the new row crosses the
    16-row block edges and the step ends in the ticket and the head merge."""
    from eetq_amd.utils.graph_decoder import GraphDecoder
    model, prompt, steps = setup["model"], setup["prompt"], setup["steps"]
    eager = GraphDecoder(model, 2, setup["max_len"], capture=False, kv_dtype="fp8_e4m3", kv_scales=(1.0, 1.0))
    rows = prompt.shape[1] + steps - 1
    a = setup["fp8"].generate(prompt, steps)
    b = eager.generate(prompt, steps)
    assert a.shape == (2, prompt.shape[1] + steps) and torch.equal(a, b)
    rows_a, rows_b = _filled(setup["fp8"], rows), _filled(eager, rows)
    blocks = [layer.self_attn for layer in model.model.layers]
    try:
        for blk in blocks:
            blk.fused_decode_step = False
        c = eager.generate(prompt, steps)
    finally:
        for blk in blocks:
            blk.fused_decode_step = True
    assert torch.equal(a, c)
    for x, y, z in zip(rows_a, rows_b, _filled(eager, rows)):
        assert torch.equal(x, y) and torch.equal(x, z)


def _logit_difference_against_the_fp16_decoder(setup):
    """Printed for DESIGN.md 4.7e, not asserted: the largest logit difference over 16 steps fed with the fp16 decoder's tokens."""
    fp16, fp8, prompt = setup["fp16"], setup["fp8"], setup["prompt"]
    worst, spread = 0.0, 0.0
    fp16.prefill(prompt)
    fp8.prefill(prompt)
    tok = prompt[:, -1:].clone()
    for step in range(16):
        for dec in (fp16, fp8):
            dec.s_tok.copy_(tok)
            dec.s_pos.fill_(prompt.shape[1] + step)
        with torch.no_grad():
            a, b = fp16._logits().float(), fp8._logits().float()
        assert torch.isfinite(b).all()
        worst, spread = max(worst, (a - b).abs().max().item()), max(spread, a.abs().max().item())
        tok = a.argmax(-1, keepdim=True)
    print("kv f8 decoder (head size %d): largest |logit(fp8 cache) - logit(fp16 cache)| over 16 steps %.4f (largest |logit| %.3f)" % (
        setup["model"].model.layers[0].self_attn.head_dim, worst, spread))


def _refusals(setup):
    import eetq_amd.modules.llama_modules as lm
    from eetq_amd.utils.graph_decoder import GraphDecoder
    model, fp8, prompt, n = setup["model"], setup["fp8"], setup["prompt"], setup["max_len"]
    for kw, names in ((dict(kv_bits=8), "kv_bits=8"), (dict(ragged=True), "ragged"), (dict(window=16), "window"),
                      (dict(window=16, rolling=True), "window"), (dict(speculative=2), "speculative")):
        with pytest.raises(ValueError, match="kv_dtype='fp8_e4m3' cannot be combined with " + names):
            GraphDecoder(model, 2, n, kv_dtype="fp8_e4m3", **kw)
    with pytest.raises(ValueError, match="kv_dtype must be"):
        GraphDecoder(model, 2, n, kv_dtype="fp8_e5m2")
    with pytest.raises(ValueError, match="kv_bits must be"):
        GraphDecoder(model, 2, n, kv_bits=4)
    with pytest.raises(ValueError, match="needs"):
        GraphDecoder(setup["stock"], 2, n, kv_dtype="fp8_e4m3")            # not an accelerated model
    for call, kw, name in ((fp8.generate, dict(append=True), "append=True"), (fp8.generate, dict(prefill_chunk=4), "prefill_chunk"),
                           (fp8.prefill, dict(append=True), "append=True"), (fp8.prefill, dict(chunk=4), "chunk")):
        with pytest.raises(ValueError, match="cannot be combined with " + name):
            call(prompt, *((4,) if call == fp8.generate else ()), **kw)
    with pytest.raises(RuntimeError, match="stock cache update"):
        fp8.cache.layers[0].update(None, None)
    # the promises an fp8 layer does not serve, at module level
    ids = torch.arange(5, device=DEV)
    promises = (lm.appended_static_prefill(), lm.appended_static_prefill(few_rows=True), lm.sliding_window_static(16),
                lm.padded_static_batch(torch.zeros(2, dtype=torch.int64, device=DEV)))
    with torch.no_grad():
        for promise in promises:
            with promise, pytest.raises(ValueError, match="an fp8 KV cache cannot be combined"):
                model(prompt[:, :5], past_key_values=fp8.cache, cache_position=ids, use_cache=True)
        with pytest.raises(NotImplementedError, match="promised fresh"):
            model(prompt[:, :5], past_key_values=fp8.cache, cache_position=ids, use_cache=True)
    k8 = torch.zeros(2, 2, 8, 64, dtype=torch.int8, device=DEV)
    q = torch.zeros(2, 4, 64, dtype=torch.float16, device=DEV)
    import eetq_amd.ops as ops
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):
        ops.decode_attention_f8kv(q, k8, k8, torch.ones(2, 2, device=DEV))


def test_fp8_decoder():
    """Each family above on both models, the family printed before it runs."""
    for head_dim in CONFIGS:
        setup = _setup(head_dim)
        for check in (_prompt_logits_cache_rows_and_set_scales, _captured_eager_and_unfused_steps,
                      _logit_difference_against_the_fp16_decoder, _refusals):
            print("head size", head_dim, check.__name__)
            check(setup)
