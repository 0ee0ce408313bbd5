"""``GraphDecoder(speculative=k, spec_attention="rows")``: the verify step's attention through ``ops.decode_attention_rows`` (the
few-row split-KV kernel) instead of the prompt kernel, on the tiny accelerated Llama of
tests/test_gpu_spec_decoder.py (hidden 256, 4 heads / 2 KV heads of 64, 2 layers, vocab 512), 96 cache rows, k = 4 -- its models,
its orbit and its argmax criterion, imported from there.

On the compiled boundary a missing ``ops.decode_attention_rows`` FAILS these tests; only the ctypes boundary skips."""
import pytest
import torch

import test_gpu_spec_decoder as base
from test_gpu_spec_decoder import cfg, cycle_model, model, perm, prompts, stock  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = base.DEV
MAX_LEN, K, VOCAB = base.MAX_LEN, base.K, base.VOCAB


@pytest.fixture(scope="module")
def ops():
    import eetq_amd.ops as o
    if o.BOUNDARY != "ext":
        pytest.skip("decode_attention_rows lives in the compiled module")
    assert o.decode_attention_rows is not None, "the compiled module lacks decode_attention_rows"
    return o


def _decoder(model, batch, capture=True, **kw):
    from eetq_amd.utils.graph_decoder import GraphDecoder
    kw.setdefault("spec_attention", "rows")
    return GraphDecoder(model, batch, MAX_LEN, capture=capture, speculative=K, **kw)


@pytest.fixture(scope="module")
def cycle_decoders(ops, cycle_model):
    return {(b, cap): _decoder(cycle_model, b, capture=cap) for b in (1, 2) for cap in (True, False)}


@pytest.mark.parametrize("capture", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("batch", [1, 2])
def test_cycle_model_tokens_and_accepted_drafts(cycle_decoders, perm, batch, capture):
    dec = cycle_decoders[(batch, capture)]
    assert dec.spec_attention == "rows"
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


def test_random_model_every_token_is_an_argmax(ops, model, prompts):
    dec = _decoder(model, 2)
    seq = dec.generate(prompts[0], 40)
    steps, tokens = dec.spec_stats()
    assert tokens == 39 and 8 <= steps <= 39 and dec.rows == 48 and base._counters(dec.cache) == [48, 48]
    assert torch.equal(dec.s_hist[:, :49], seq)
    base._assert_every_token_is_an_argmax(model, seq, range(9, 49), "rows attention, lookup drafts (%d steps for 39 tokens)" % steps)


def test_sampled_verification(ops, cycle_model, cycle_decoders, perm):
    """spec_sampling=True verification runs on the rows kernel, and at temperature 0 it is the greedy decoder"""
    dec = _decoder(cycle_model, 2, sampling=True, spec_sampling=True)
    rows = [[first] + base._orbit(perm, first, 8) for first in (10, 23)]
    prompt = torch.tensor(rows, device=DEV)
    greedy = cycle_decoders[(2, True)].generate(prompt, 23)
    assert torch.equal(dec.generate(prompt, 23, do_sample=True, temperature=0.0, seed=5), greedy)
    assert dec.spec_stats() == (5, 22)
    assert torch.equal(dec.generate(prompt, 23), greedy)                             # do_sample=False
    drawn = dec.generate(prompt, 23, do_sample=True, temperature=0.6, seed=5)
    assert drawn.shape == (2, 32) and torch.equal(drawn, dec.generate(prompt, 23, do_sample=True, temperature=0.6, seed=5))


def _ready_for_one_step(dec, prompt):
    """the state generate(prompt, K + 2) has before its first verify step (the prompt runs on the prompt kernel, whatever the mode)"""
    dec.generate(prompt, 1)
    dec.s_limit.fill_(K + 2)


def _count_calls(monkeypatch, ops):
    calls = {"rows": 0, "prompt": 0}
    rows_op, prompt_op = ops.decode_attention_rows, ops.prefill_attention

    def rows(*a, **kw):
        calls["rows"] += 1
        return rows_op(*a, **kw)

    def prompt(*a, **kw):
        calls["prompt"] += 1
        return prompt_op(*a, **kw)

    monkeypatch.setattr(ops, "decode_attention_rows", rows)
    monkeypatch.setattr(ops, "prefill_attention", prompt)
    return calls


@pytest.mark.parametrize("mode", ["rows", "prompt"])
def test_the_kernel_is_actually_used(ops, model, prompts, monkeypatch, mode):
    """one eager verify step: once per layer through the chosen operator, never through the other"""
    dec = _decoder(model, 2, capture=False, spec_attention=mode)
    _ready_for_one_step(dec, prompts[0])
    calls = _count_calls(monkeypatch, ops)
    dec._advance_spec()
    layers = len(model.model.layers)
    assert calls == ({"rows": layers, "prompt": 0} if mode == "rows" else {"rows": 0, "prompt": layers}), calls


def test_logits_agree_with_the_prompt_kernel(ops, model, prompts):
    """one eager verify step from the same cache state under "rows" and under "prompt": the logits within twice the tolerance"""
    got = {}
    for mode in ("rows", "prompt"):
        dec = _decoder(model, 2, capture=False, spec_attention=mode)
        _ready_for_one_step(dec, prompts[0])
        seen = []
        hook = model.lm_head.register_forward_hook(lambda mod, args, out, _seen=seen: _seen.append(out.float().clone()))
        try:
            dec._advance_spec()
        finally:
            hook.remove()
        assert len(seen) == 1 and seen[0].shape == (2, K + 1, VOCAB)
        got[mode] = seen[0]
    tol = 2 * base._tol(got["prompt"])
    worst = (got["rows"] - got["prompt"]).abs().max().item()
    print("spec rows decoder: verify-step logits, rows against prompt: %.3g of %.3g" % (worst, tol))
    assert worst <= tol and not torch.isnan(got["rows"]).any()


def test_argument_checks(ops, model, monkeypatch):
    from eetq_amd.modules.llama_modules import appended_static_prefill, padded_static_batch
    from eetq_amd.utils.graph_decoder import GraphDecoder
    for bad in ("auto", "", None, 1):
        with pytest.raises(ValueError, match="spec_attention must be"):
            GraphDecoder(model, 2, MAX_LEN, speculative=K, spec_attention=bad)
    with pytest.raises(ValueError, match="needs a speculative decoder"):
        GraphDecoder(model, 2, MAX_LEN, spec_attention="rows")
    with pytest.raises(ValueError, match="fp16 cache rows only"):
        with appended_static_prefill(int8_rows=True, few_rows=True):
            pass
    starts = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="one shared first key only"):
        with padded_static_batch(starts):
            with appended_static_prefill(few_rows=True):
                pass
    with pytest.raises(ValueError, match="one shared first key only"):
        with appended_static_prefill(few_rows=True):
            with padded_static_batch(starts):
                pass
    with appended_static_prefill(few_rows=True):                 # restored on exit, like the other promises
        pass
    with padded_static_batch(starts):
        pass
    monkeypatch.setattr(ops, "decode_attention_rows", None)
    with pytest.raises(ValueError, match="compiled operator module"):
        GraphDecoder(model, 2, MAX_LEN, speculative=K, spec_attention="rows")


def test_default_is_unchanged(ops, model, prompts):
    """a decoder built without the argument produces the same tokens alone and next to a "rows" decoder of the same model"""
    from eetq_amd.utils.graph_decoder import GraphDecoder
    alone = GraphDecoder(model, 2, MAX_LEN, speculative=K)
    assert alone.spec_attention == "prompt"
    before = alone.generate(prompts[0], 30)
    stats = alone.spec_stats()
    rows = _decoder(model, 2)
    rows.generate(prompts[0], 30)
    again = alone.generate(prompts[0], 30)
    assert torch.equal(before, again) and alone.spec_stats() == stats
    other = GraphDecoder(model, 2, MAX_LEN, speculative=K)
    assert torch.equal(other.generate(prompts[0], 30), before)
