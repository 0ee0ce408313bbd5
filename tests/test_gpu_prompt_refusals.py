"""The argument refusals of the prompt-side operators, word for word: prefill_attention, prefill_attention_i8kv and
decode_attention_rows (torch_ext.cpp: PromptAttnPrep and the checks in front of it) and the two cache-writing rotary prompt
operators in BOTH bindings (torch_ext.cpp and ops_ctypes.py: the shared preparation and the cache check handed to it).  One call
per requirement; every call asserts the WHOLE message, and a call that breaks two requirements at once pins which of them is
reported -- the order of the checks is part of the operators' behaviour.

B = 2, H = 4, Hkv = 2, D = 64, T = 3, 8 cache rows, zeros: a refusal happens before anything is launched, so the values do not
matter.  The last test calls every operator with its valid arguments: the cases above are refused for the stated reason alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, HKV, D, T, S = 2, 4, 2, 64, 3, 8
ATTN = ("prefill_attention", "prefill_attention_i8kv", "decode_attention_rows")
ROTARY = ("rotary_embedding_neox_kvcache_prefill", "rotary_embedding_neox_kvcache_prefill_i8")
MAX_SPLITS = {"prefill_attention": 16, "prefill_attention_i8kv": 16, "decode_attention_rows": 64}
# workspace floats at splits = 2 (B H T splits (D + 2) and B H R splits (D + 4)) and at the library's own count for this shape (1)
NEED2 = {"prefill_attention": 3168, "prefill_attention_i8kv": 3168, "decode_attention_rows": 3264}
NEED_DEFAULT = {"prefill_attention": 0, "prefill_attention_i8kv": 0, "decode_attention_rows": 1632}


def _half(*shape, device=DEV):
    return torch.zeros(shape, dtype=torch.float16, device=device)


def _i64(*values, device=DEV):
    return torch.tensor(values, dtype=torch.int64, device=device)


def _i8_caches():
    return {"key_cache": torch.zeros(B, HKV, S, D, dtype=torch.int8, device=DEV),
            "value_cache": torch.zeros(B, HKV, S, D, dtype=torch.int8, device=DEV), "scales": _half(B, HKV, S, 2)}


def _attn_args(op):
    if op == "prefill_attention_i8kv":
        return {"query": _half(B, T, H, D), **_i8_caches(), "max_keys": S}
    return {"query": _half(B, T, H, D), "key": _half(B, HKV, S, D), "value": _half(B, HKV, S, D), "keys": S}


def _rotary_args(op):
    kw = {"positions": torch.zeros(B, T, dtype=torch.int64, device=DEV), "query": _half(B, T, H, D), "key": _half(B, T, HKV, D),
          "value": _half(B, T, HKV, D), "head_size": D, "cos_sin_cache": _half(16, D)}
    if op.endswith("_i8"):
        kw.update(_i8_caches())
    else:
        kw.update(key_cache=_half(B, HKV, S, D), value_cache=_half(B, HKV, S, D))
    return kw


def _message(err):
    """the operator's message: the compiled module may append the C++ frames behind it"""
    return str(err.value).split("\nException raised from")[0]


def _put(**values):   # a callable value is made when the case runs: nothing here touches the GPU at import
    return lambda op, kw: kw.update({k: v() if callable(v) else v for k, v in values.items()})


def _change(name, make):
    def mutate(op, kw):
        kw[name] = make(kw[name])
    return mutate


def _both(*mutations):
    def mutate(op, kw):
        for m in mutations:
            m(op, kw)
    return mutate


def _cache_names(op):
    return ("key", "value") if op in ("prefill_attention", "decode_attention_rows") else ("key_cache", "value_cache")


def _caches(make):   # both caches alike
    def mutate(op, kw):
        for n in _cache_names(op):
            kw[n] = make(kw[n])
    return mutate


def _workspace(make, **more):
    def mutate(op, kw):
        kw.update(more)
        kw["workspace"] = make(NEED2[op])
    return mutate


KV_LEN = "kv_len must be a one-element int64 tensor on the query's device"
SPLITS = lambda op: "splits must lie in 1 .. %d" % MAX_SPLITS[op]                                            # noqa: E731
WS2 = lambda op: "workspace must be a contiguous float32 tensor of at least %d elements on the query's device" % NEED2[op]  # noqa: E731
WS1 = lambda op: ("workspace must be a contiguous float32 tensor of at least %d elements on the query's device"
                  % NEED_DEFAULT[op])                                                                       # noqa: E731
TENSORS = lambda op: ("float16 CUDA tensors [B, %s, H, D] / [B, Hkv, S, D] with a dense last dimension expected"
                      % ("R" if op == "decode_attention_rows" else "T"))                                    # noqa: E731
ROWS = lambda n: "1 .. 16 query rows per batch row (got %d)" % n                                            # noqa: E731

# (id, operators, mutation of the valid arguments, the text behind "operator: ")
ATTN_CASES = [
    ("bias-without-kv_len", ATTN, _put(kv_len_bias=1), "kv_len_bias needs kv_len"),
    ("kv_len-int32", ATTN, _put(kv_len=lambda: torch.tensor([S], dtype=torch.int32, device=DEV)), KV_LEN),
    ("kv_len-two-elements", ATTN, _put(kv_len=lambda: _i64(S, S)), KV_LEN),
    ("kv_len-on-the-host", ATTN, _put(kv_len=lambda: _i64(S, device="cpu")), KV_LEN),
    ("splits-0", ATTN, _put(splits=0), SPLITS),
    ("splits-beyond", ATTN, lambda op, kw: kw.update(splits=MAX_SPLITS[op] + 1), SPLITS),
    ("workspace-float64", ATTN, _workspace(lambda n: torch.zeros(n, dtype=torch.float64, device=DEV), splits=2), WS2),
    ("workspace-short", ATTN, _workspace(lambda n: torch.zeros(n - 1, device=DEV), splits=2), WS2),
    ("workspace-strided", ATTN, _workspace(lambda n: torch.zeros(2 * n, device=DEV)[::2], splits=2), WS2),
    ("workspace-on-the-host", ATTN, _workspace(lambda n: torch.zeros(n), splits=2), WS2),
    ("workspace-float64-default-splits", ATTN, _workspace(lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)), WS1),
    ("query-float32", (ATTN[0], ATTN[2]), _change("query", lambda t: t.float()), TENSORS),
    ("query-3d", (ATTN[0], ATTN[2]), _change("query", lambda t: t[0]), TENSORS),
    ("key-strided-channels", (ATTN[0], ATTN[2]), _change("key", lambda t: _half(B, HKV, S, 2 * D)[..., ::2]), TENSORS),
    ("value-on-the-host", (ATTN[0], ATTN[2]), _change("value", lambda t: t.cpu()), TENSORS),
    ("query-float32", (ATTN[1],), _change("query", lambda t: t.float()), "expected a float16 CUDA query [B, T, H, D] with dense D"),
    ("keys-beyond-the-cache", (ATTN[0], ATTN[2]), _put(keys=S + 1), "shape mismatch"),
    ("keys-beyond-the-cache", (ATTN[1],), _put(max_keys=S + 1), "shape mismatch"),
    ("keys-0", (ATTN[0], ATTN[2]), _put(keys=0), "shape mismatch"),
    ("keys-0", (ATTN[1],), _put(max_keys=0), "shape mismatch"),
    ("value-other-shape", (ATTN[0], ATTN[2]), _change("value", lambda t: _half(B, HKV, S + 1, D)), "shape mismatch"),
    ("three-kv-heads", ATTN, _both(_caches(lambda t: torch.zeros(B, 3, S, D, dtype=t.dtype, device=DEV)),
                                   lambda op, kw: kw.update(scales=_half(B, 3, S, 2)) if "i8" in op else None), "shape mismatch"),
    ("no-query-rows", (ATTN[0], ATTN[1]), _change("query", lambda t: _half(B, 0, H, D)), "shape mismatch"),
    ("no-query-rows", (ATTN[2],), _change("query", lambda t: _half(B, 0, H, D)), ROWS(0)),
    ("seventeen-rows", (ATTN[2],), _change("query", lambda t: _half(B, 17, H, D)), ROWS(17)),
    ("empty-batch", (ATTN[2],), _both(_change("query", lambda t: _half(0, T, H, D)), _caches(lambda t: _half(0, HKV, S, D))),
     "shape mismatch"),
    ("head-size-32", ATTN, _both(_change("query", lambda t: _half(B, T, H, 32)),
                                 _caches(lambda t: torch.zeros(B, HKV, S, 32, dtype=t.dtype, device=DEV))), "unsupported head_dim"),
    ("kv_len-with-causal_offset", (ATTN[0],), _put(kv_len=lambda: _i64(S), causal_offset=0),
     "kv_len and causal_offset exclude each other (with kv_len the offset is the device length minus the query rows)"),
    ("kv_start-int32", (ATTN[0],), _put(kv_start=lambda: torch.zeros(B, dtype=torch.int32, device=DEV)),
     "kv_start must be a contiguous int64 [B] tensor on the query's device"),
    ("int8-caches-as-float16", (ATTN[1],), _caches(lambda t: t.half()), "the caches must be int8 and the scales float16"),
    # two requirements at once: the one the operator reports
    ("bias-and-splits-0", ATTN, _put(kv_len_bias=1, splits=0), "kv_len_bias needs kv_len"),
    ("kv_len-int32-and-splits-beyond", ATTN, _put(kv_len=lambda: torch.tensor([S], dtype=torch.int32, device=DEV), splits=65), KV_LEN),
    ("splits-0-and-workspace-float64", ATTN, _put(splits=0, workspace=lambda: torch.zeros(8, dtype=torch.float64, device=DEV)), SPLITS),
    ("keys-0-and-bias", ATTN, lambda op, kw: kw.update({"max_keys" if "i8" in op else "keys": 0, "kv_len_bias": 1}), "shape mismatch"),
    ("head-size-32-and-bias", ATTN, _both(_change("query", lambda t: _half(B, T, H, 32)),
                                          _caches(lambda t: torch.zeros(B, HKV, S, 32, dtype=t.dtype, device=DEV)), _put(kv_len_bias=1)),
     "unsupported head_dim"),
    ("query-float32-and-keys-0", (ATTN[0], ATTN[2]), _both(_change("query", lambda t: t.float()), _put(keys=0)), TENSORS),
    ("seventeen-rows-and-bias", (ATTN[2],), _both(_change("query", lambda t: _half(B, 17, H, D)), _put(kv_len_bias=1)), ROWS(17)),
    ("kv_start-int32-and-bias", (ATTN[0],), _put(kv_start=lambda: torch.zeros(B, dtype=torch.int32, device=DEV), kv_len_bias=1),
     "kv_start must be a contiguous int64 [B] tensor on the query's device"),
    ("causal_offset-and-bad-kv_len", (ATTN[0],), _put(kv_len=lambda: _i64(S, S), causal_offset=0),
     "kv_len and causal_offset exclude each other (with kv_len the offset is the device length minus the query rows)"),
    ("int8-caches-as-float16-and-bias", (ATTN[1],), _both(_caches(lambda t: t.half()), _put(kv_len_bias=1)),
     "the caches must be int8 and the scales float16"),
]

HALVES = lambda op: "float16 query, key, value and cos|sin table expected" if op.endswith("_i8") else "float16 tensors expected"  # noqa: E731
TABLE = lambda op: "the cos|sin table must be contiguous" if op.endswith("_i8") else "cache rows must be dense"                 # noqa: E731
ONE_DEVICE = "all tensors must be on one CUDA device"
TOKENS = "[heads, head_size] must be dense and the tokens of all rows one stride apart"
FIRST_ROW_DEV = "first_row_dev must be one int64 on the device"
I8_LAYOUT = "expected caches [B, Hkv, S, D] and scales [B, Hkv, S, 2]"


def _strided_rows(t):   # the same sizes, other strides, dense channels
    return torch.zeros(B, HKV, 2 * S, D, dtype=t.dtype, device=DEV)[:, :, ::2]


def _strided_channels(t):
    return torch.zeros(B, HKV, S, 2 * D, dtype=t.dtype, device=DEV)[..., ::2]


ROTARY_CASES = [
    ("query-float32", ROTARY, _change("query", lambda t: t.float()), HALVES),
    ("table-float32", ROTARY, _change("cos_sin_cache", lambda t: t.float()), HALVES),
    ("value-on-the-host", ROTARY, _change("value", lambda t: t.cpu()), ONE_DEVICE),
    ("key_cache-float32", (ROTARY[0],), _change("key_cache", lambda t: t.float()), "float16 tensors expected"),
    ("key_cache-float16", (ROTARY[1],), _change("key_cache", lambda t: t.half()), "the caches must be int8 and the scales float16"),
    ("value_cache-on-the-host", (ROTARY[0],), _change("value_cache", lambda t: t.cpu()), ONE_DEVICE),
    ("value_cache-on-the-host", (ROTARY[1],), _change("value_cache", lambda t: t.cpu()), "all tensors must be on one device"),
    ("positions-int32", ROTARY, _change("positions", lambda t: t.int()), "positions must be contiguous int64 on the device"),
    ("positions-strided", ROTARY, _change("positions", lambda t: torch.zeros(B, 2 * T, dtype=torch.int64, device=DEV)[:, ::2]),
     "positions must be contiguous int64 on the device"),
    ("positions-on-the-host", ROTARY, _change("positions", lambda t: t.cpu()), "positions must be contiguous int64 on the device"),
    ("key-3d", ROTARY, _change("key", lambda t: t[0]), "shape mismatch"),
    ("key_cache-3d", (ROTARY[0],), _change("key_cache", lambda t: t[0]), "shape mismatch"),
    ("key-other-heads", ROTARY, _change("key", lambda t: _half(B, T, 1, D)), "shape mismatch"),
    ("key-other-tokens", ROTARY, _change("key", lambda t: _half(B, T + 1, HKV, D)), "shape mismatch"),
    ("value-other-shape", ROTARY, _change("value", lambda t: _half(B, T + 1, HKV, D)), "shape mismatch"),
    ("head_size-other", ROTARY, _put(head_size=D // 2), "shape mismatch"),
    ("cache-other-batch", (ROTARY[0],), _both(_change("key_cache", lambda t: _half(1, HKV, S, D)),
                                               _change("value_cache", lambda t: _half(1, HKV, S, D))), "shape mismatch"),
    ("value_cache-other-shape", (ROTARY[0],), _change("value_cache", lambda t: _half(B, HKV, S + 1, D)), "shape mismatch"),
    ("value_cache-other-shape", (ROTARY[1],), _change("value_cache", lambda t: torch.zeros(B, HKV, S + 1, D, dtype=torch.int8, device=DEV)),
     I8_LAYOUT),
    ("scales-3d", (ROTARY[1],), _change("scales", lambda t: t[0]), I8_LAYOUT),
    ("scales-three-wide", (ROTARY[1],), _change("scales", lambda t: _half(B, HKV, S, 3)), "shape mismatch"),
    ("value_cache-other-strides", ROTARY, _change("value_cache", _strided_rows), "shape mismatch"),
    ("positions-short", ROTARY, _change("positions", lambda t: t[:, :1].contiguous()), "shape mismatch"),
    ("first_row-negative", ROTARY, _put(first_row=-1), "shape mismatch"),
    ("first_row-beyond", ROTARY, _put(first_row=S - T + 1), "shape mismatch"),
    ("first_row_dev-int32", ROTARY, _put(first_row_dev=lambda: torch.zeros(1, dtype=torch.int32, device=DEV)), FIRST_ROW_DEV),
    ("first_row_dev-two-elements", ROTARY, _put(first_row_dev=lambda: _i64(0, 0)), FIRST_ROW_DEV),
    ("first_row_dev-on-the-host", ROTARY, _put(first_row_dev=lambda: _i64(0, device="cpu")), FIRST_ROW_DEV),
    ("query-padded-heads", ROTARY, _change("query", lambda t: _half(B, T, H, 2 * D)[..., :D]), TOKENS),
    ("value-strided-channels", ROTARY, _change("value", lambda t: _half(B, T, HKV, 2 * D)[..., ::2]), TOKENS),
    ("key-rows-apart", ROTARY, _change("key", lambda t: _half(B, 2 * T, HKV, D)[:, :T]), TOKENS),
    ("table-strided", ROTARY, _change("cos_sin_cache", lambda t: _half(16, 2 * D)[:, :D]), TABLE),
    ("caches-strided-channels", (ROTARY[0],), _caches(_strided_channels), "cache rows must be dense"),
    ("caches-strided-channels", (ROTARY[1],), _caches(_strided_channels), "cache rows and scale pairs must be dense"),
    # two requirements at once: the one the operator reports
    ("key-on-the-host-and-value-float32", ROTARY, _both(_change("key", lambda t: t.cpu()), _change("value", lambda t: t.float())),
     ONE_DEVICE),
    ("value-float32-and-positions-int32", ROTARY, _both(_change("value", lambda t: t.float()), _change("positions", lambda t: t.int())),
     HALVES),
    ("positions-int32-and-key-3d", ROTARY, _both(_change("positions", lambda t: t.int()), _change("key", lambda t: t[0])),
     "positions must be contiguous int64 on the device"),
    ("scales-3d-and-head_size-other", (ROTARY[1],), _both(_change("scales", lambda t: t[0]), _put(head_size=D // 2)), I8_LAYOUT),
    ("caches-strided-channels-and-first_row-beyond", (ROTARY[1],), _both(_caches(_strided_channels), _put(first_row=S)),
     "cache rows and scale pairs must be dense"),
    ("caches-strided-channels-and-first_row_dev-int32", (ROTARY[0],),
     _both(_caches(_strided_channels), _put(first_row_dev=lambda: torch.zeros(1, dtype=torch.int32, device=DEV))), FIRST_ROW_DEV),
    ("first_row-negative-and-first_row_dev-int32", ROTARY, _put(first_row=-1, first_row_dev=lambda: torch.zeros(1, dtype=torch.int32, device=DEV)),
     "shape mismatch"),
    ("first_row_dev-int32-and-query-padded-heads", ROTARY,
     _both(_put(first_row_dev=lambda: torch.zeros(1, dtype=torch.int32, device=DEV)), _change("query", lambda t: _half(B, T, H, 2 * D)[..., :D])),
     FIRST_ROW_DEV),
    ("query-padded-heads-and-table-strided", ROTARY,
     _both(_change("query", lambda t: _half(B, T, H, 2 * D)[..., :D]), _change("cos_sin_cache", lambda t: _half(16, 2 * D)[:, :D])), TOKENS),
]


def _flat(cases):
    return [pytest.param(op, mutate, text, id="%s-%s" % (op, cid)) for cid, ops_, mutate, text in cases for op in ops_]


def _refused(fn, name, kw, mutate, text):
    mutate(name, kw)
    with pytest.raises(RuntimeError) as err:
        fn(**kw)
    assert _message(err) == "%s: %s" % (name, text(name) if callable(text) else text)


@pytest.mark.parametrize("op,mutate,text", _flat(ATTN_CASES))
def test_attention_refusal(op, mutate, text):
    from eetq_amd import ops
    _refused(getattr(ops, op), op, _attn_args(op), mutate, text)


@pytest.mark.parametrize("binding", ("ext", "ctypes"))
@pytest.mark.parametrize("op,mutate,text", _flat(ROTARY_CASES))
def test_rotary_prefill_refusal(binding, op, mutate, text):
    from eetq_amd import _ext, ops_ctypes
    _refused(getattr(_ext.load() if binding == "ext" else ops_ctypes, op), op, _rotary_args(op), mutate, text)


def test_valid_arguments_are_accepted():
    from eetq_amd import _ext, ops, ops_ctypes
    for op in ATTN:
        out = getattr(ops, op)(**_attn_args(op))
        assert out.shape == (B, T, H, D) and bool((out == 0).all())
        out = getattr(ops, op)(**_attn_args(op), kv_len=_i64(S), kv_len_bias=-1, splits=2,
                               workspace=torch.zeros(NEED2[op], device=DEV))
        assert out.shape == (B, T, H, D) and bool((out == 0).all())
    for binding in (_ext.load(), ops_ctypes):
        for op in ROTARY:
            kw = _rotary_args(op)
            assert getattr(binding, op)(**kw, first_row=S - T) is None
            assert getattr(binding, op)(**kw, first_row_dev=_i64(1)) is None
    torch.cuda.synchronize()
