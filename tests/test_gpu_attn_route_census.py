"""Which operators one attention-module forward reaches under every promise, on an fp16 and on an int8 static cache.

The model is the tiny accelerated Llama of tests/test_gpu_window_decoder.py cut down to one layer (hidden 128, 2 heads / 1 KV head,
head size 64, vocab 64), batch 2, 64 cache rows.  ``llama_modules.ops`` is replaced by a proxy that forwards every attribute to the
real module and logs each call: the operator's name, which of ``kv_len`` / ``kv_start`` / ``window`` / ``first_row_dev`` it was given,
and the ``keys`` argument of the prompt and few-row operators.  Every case starts from a fresh 5-token prompt and then runs ONE
forward of the attention module; the sequence of calls and those arguments are asserted, nothing else -- the numbers are the
decoder tests'.  Every refusal here is raised on the host before any launch."""
import contextlib
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, ROWS, SEEN, HIDDEN = 2, 64, 5, 128
GIVEN = ("kv_len", "kv_start", "window", "first_row_dev")
KEYS_AT = {"prefill_attention": 3, "decode_attention_rows": 3, "prefill_attention_i8kv": 4, "decode_attention_rows_i8kv": 4}


class OpsProxy:
    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        op = getattr(self._real, name)
        if not callable(op) or name.endswith("_supported"):     # a missing operator stays None; a predicate launches nothing
            return op

        def logged(*args, **kwargs):
            keys = args[KEYS_AT[name]] if name in KEYS_AT else None
            self._log.append((name, tuple(g for g in GIVEN if kwargs.get(g) is not None), keys))
            return op(*args, **kwargs)
        return logged


@pytest.fixture(scope="module")
def setup():
    transformers = pytest.importorskip("transformers")
    from eetq_amd.utils import eet_accelerator
    from eetq_amd.utils.kv_cache import Int8StaticCache
    cfg = transformers.LlamaConfig(hidden_size=HIDDEN, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                                   num_key_value_heads=1, vocab_size=64, max_position_embeddings=128, attn_implementation="eager")
    torch.manual_seed(0)
    stock = transformers.LlamaForCausalLM(cfg).half().to(DEV).eval()
    model = eet_accelerator(copy.deepcopy(stock), quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)
    fp16 = transformers.StaticCache(config=cfg, max_cache_len=ROWS)
    with torch.no_grad():   # the fp16 cache allocates its rows in its first forward
        model(torch.zeros(B, 1, dtype=torch.long, device=DEV), past_key_values=fp16, cache_position=torch.zeros(1, dtype=torch.long, device=DEV),
              use_cache=True)
    int8 = Int8StaticCache(config=cfg, max_cache_len=ROWS).allocate(B, DEV)
    g = torch.Generator().manual_seed(3)
    hidden = torch.randn(B, 32, HIDDEN, generator=g).half().to(DEV)
    return model.model.layers[0].self_attn, {"fp16": fp16, "int8": int8}, hidden


@pytest.fixture
def run(setup, monkeypatch):
    import eetq_amd.modules.llama_modules as lm
    attn, caches, hidden = setup
    log = []
    monkeypatch.setattr(lm, "ops", OpsProxy(lm.ops, log))
    starts = torch.tensor([1, 0], dtype=torch.int64, device=DEV)

    def forward(cache, t_len, first, promises):
        pos = (torch.arange(t_len, device=DEV) + first)[None, :].expand(B, t_len)
        with contextlib.ExitStack() as stack, torch.no_grad():
            for p in promises:
                stack.enter_context(p)
            attn(hidden[:, first: first + t_len].contiguous(), attention_mask=None, position_ids=pos, past_key_values=caches[cache])

    def census(cache, t_len, *promises, fresh=False):
        """the calls of one forward of `t_len` rows behind a fresh 5-token prompt (`fresh`: of one more fresh prompt)"""
        caches[cache].reset()
        forward(cache, SEEN, 0, [lm.fresh_static_prefill()])
        del log[:]
        forward(cache, t_len, 0 if fresh else SEEN, promises)
        return list(log)

    census.lm, census.attn, census.starts, census.log = lm, attn, starts, log
    return census


WRITE, PROMPT, ROWS_OP = "rotary_embedding_neox_kvcache_prefill", "prefill_attention", "decode_attention_rows"


@pytest.mark.parametrize("extra", (None, "window", "kv_start"))
def test_fp16_prompts(run, extra):
    lm = run.lm
    also = {None: lambda: [], "window": lambda: [lm.sliding_window_static(3)], "kv_start": lambda: [lm.padded_static_batch(run.starts)]}[extra]
    more = () if extra is None else (extra,)
    assert run("fp16", 5, lm.fresh_static_prefill(), *also(), fresh=True) == [(WRITE, (), None), (PROMPT, more, 5)]
    order = tuple(g for g in GIVEN if g in ("kv_len",) + more)
    assert run("fp16", 5, lm.appended_static_prefill(), *also()) == [(WRITE, ("first_row_dev",), None), (PROMPT, order, ROWS)]


def test_fp16_few_rows_and_no_promise(run):
    lm = run.lm
    write = (WRITE, ("first_row_dev",), None)
    for t_len in (2, 16):
        assert run("fp16", t_len, lm.appended_static_prefill(few_rows=True)) == [write, (ROWS_OP, ("kv_len",), ROWS)]
    assert run("fp16", 17, lm.appended_static_prefill(few_rows=True)) == [write, (PROMPT, ("kv_len",), ROWS)]
    assert run("fp16", 5) == [write]          # no promise: the write, then the stock attention path


def test_fp16_single_token(run, monkeypatch):
    lm = run.lm
    assert run("fp16", 1) == [("rope_decode_attention", ("kv_len",), None)]
    assert run("fp16", 1, lm.padded_static_batch(run.starts)) == [("rope_decode_attention", ("kv_len", "kv_start"), None)]
    assert run("fp16", 1, lm.sliding_window_static(3)) == [("rope_decode_attention", ("kv_len", "window"), None)]
    monkeypatch.setattr(run.attn, "fused_decode_step", False)
    assert run("fp16", 1) == [("rotary_embedding_neox_kvcache", (), None), ("decode_attention", ("kv_len",), None)]


def test_int8_cache(run):
    lm = run.lm
    write8 = "rotary_embedding_neox_kvcache_prefill_i8"
    assert run("int8", 5, lm.fresh_static_prefill(), fresh=True) == [(write8, (), None), (PROMPT, (), 5)]
    behind = (write8, ("first_row_dev",), None)
    assert run("int8", 5, lm.appended_static_prefill(int8_rows=True)) == [behind, ("prefill_attention_i8kv", ("kv_len",), ROWS)]
    for t_len in (2, 16):
        assert run("int8", t_len, lm.appended_static_prefill(int8_rows=True, few_rows_int8=True)) == [
            behind, ("decode_attention_rows_i8kv", ("kv_len",), ROWS)]
    assert run("int8", 17, lm.appended_static_prefill(int8_rows=True, few_rows_int8=True)) == [
        behind, ("prefill_attention_i8kv", ("kv_len",), ROWS)]
    assert run("int8", 1) == [("rope_decode_attention_i8kv", ("kv_len",), None)]


def test_int8_refusals_launch_nothing(run):
    lm = run.lm
    for promises in ((), (lm.appended_static_prefill(),)):
        with pytest.raises(NotImplementedError):
            run("int8", 5, *promises)
        assert run.log == []
    with pytest.raises(ValueError, match="sliding_window_static"):
        run("int8", 5, lm.fresh_static_prefill(), lm.sliding_window_static(3), fresh=True)
    with pytest.raises(ValueError, match="padded_static_batch"):
        run("int8", 5, lm.fresh_static_prefill(), lm.padded_static_batch(run.starts), fresh=True)
    assert run.log == []
