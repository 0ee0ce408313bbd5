"""The int8 KV cache without a GPU: the NumPy row quantiser the GPU tests use as their reference (tests/kv8_cases.py), the three
entry points in the header and in the library, their refusals (which come before any launch), and the cache classes."""
import ctypes
import os
import re

import numpy as np
import pytest

import attn_cases as ac
import kv8_cases as k8c

ERR_INVALID, ERR_UNSUPPORTED = -1, -3
ENTRIES = ("eetq_decode_attention_i8kv_f16", "eetq_rope_decode_attention_i8kv_f16", "eetq_rotary_neox_kvcache_prefill_i8_f16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the NumPy quantiser -----------------------------------------------------------------------------------------------------
def test_quantiser_on_normal_rows():
    rng = np.random.default_rng(0)
    for D in (64, 128):
        x = ac.normal_f16(rng, (4096, D))
        q, s = k8c.quantize_rows(x)
        assert q.dtype == np.int8 and s.dtype == np.float16
        assert np.abs(q.astype(np.int32)).max(-1).min() == 127 and np.abs(q.astype(np.int32)).max() == 127   # never -128
        amax = np.abs(x.astype(np.float64)).max(-1)
        assert np.array_equal(s, (amax.astype(np.float32) * (np.float32(1) / np.float32(127))).astype(np.float16))
        # amax / s: fp16 rounds the scale by at most 2^-11 relative (normal range), so the ratio lies in 127 / (1 + 2^-11) ..
        # 127 (1 + 2^-11) = 126.938 .. 127.062; to the two decimals the figures are quoted with, 126.94 .. 127.06
        ratio = amax / s.astype(np.float64)
        assert 127 / (1 + 2.0 ** -11) <= ratio.min() and ratio.max() <= 127 * (1 + 2.0 ** -11), (ratio.min(), ratio.max())
        assert round(ratio.min(), 2) >= 126.94 and round(ratio.max(), 2) <= 127.06, (ratio.min(), ratio.max())
        err = np.abs(k8c.dequantize_rows(q, s) - x.astype(np.float64))
        assert (err <= 0.5 * s.astype(np.float64)[:, None] * (1 + 2.0 ** -20) + 2.0 ** -30).all()


def test_quantiser_edge_rows():
    zero = np.zeros((1, 64), dtype=np.float16)
    q, s = k8c.quantize_rows(zero)
    assert s[0] == 0 and not q.any()
    # exact halves round away from zero: scale 1 (amax 127), elements k + 0.5
    row = np.zeros((1, 64), dtype=np.float16)
    row[0, :8] = [127, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 63.5]
    q, s = k8c.quantize_rows(row)
    assert s[0] == 1 and q[0, :8].tolist() == [127, 1, -1, 2, -2, 3, -3, 64]
    # a negative extreme is -127, and a value beyond 127 steps is clamped (a scale that rounded down)
    row = np.full((1, 64), 0.25, dtype=np.float16)
    row[0, 5] = -3.0
    q, s = k8c.quantize_rows(row)
    assert q[0, 5] == -127 and q.min() == -127
    for bits in range(0x3C00, 0x4400, 7):
        a = np.array([bits], dtype=np.uint16).view(np.float16)
        q, s = k8c.quantize_rows(np.concatenate([a, np.zeros(63, dtype=np.float16)])[None])
        assert q[0, 0] == 127, (bits, s)
    assert k8c.hot_value(np.array([[3, -5]], dtype=np.int8), np.array([0.5], dtype=np.float16)).tolist() == [[1.5, -2.5]]


def test_edge_row_builders_deliver_what_the_gpu_tests_rely_on():
    """tests/test_gpu_kv8_edges.py feeds `edge_rows` to the GPU writers and expects `quantize_rows` of them.  Pinned here, on the
    NumPy quantiser alone: the tie rows are ties, the tiny rows reach the subnormal scales and the clamp, every sweep row
    peaks at its own channel under a scale of its own."""
    total = 0
    for D in (64, 128):
        fam = k8c.edge_rows(D)
        rows, where = k8c.edge_rows_flat(D)
        assert rows.dtype == np.float16 and rows.shape == (sum(len(r) for r in fam.values()), D)
        assert list(fam) == ["ties", "tiny", "extreme", "sweep", "zero"] and np.isfinite(rows.astype(np.float64)).all()
        assert not (np.signbit(rows) & (rows == 0)).any(), "no -0: the identity rotation returns the row bit for bit"
        total += len(rows)
        # ties: scale 2^e exactly, every other element an exact k + 0.5 quotient, every k with both signs, away from zero
        t = fam["ties"]
        q, s = k8c.quantize_rows(t)
        per_e = len(t) // len(k8c.TIE_EXPONENTS)
        assert len(t) == 2 * len(k8c.TIE_EXPONENTS) * -(-127 // (D - 1))
        seen = set()
        for i, e in enumerate(k8c.TIE_EXPONENTS):
            blk = slice(i * per_e, (i + 1) * per_e)
            assert (s[blk].astype(np.float64) == 2.0 ** e).all()
            r = t[blk].astype(np.float32) / s[blk].astype(np.float32)[:, None]          # the quantiser's own fp32 quotient
            assert (np.abs(r[:, 0]) == 127).all() and (np.abs(q[blk][:, 0]) == 127).all()
            frac = np.abs(r[:, 1:]).astype(np.float64)
            assert (frac - np.floor(frac) == 0.5).all(), "exact halves"
            assert (np.abs(q[blk][:, 1:].astype(np.float64)) == np.floor(frac) + 1).all() and (np.sign(q[blk][:, 1:]) == np.sign(r[:, 1:])).all()
            seen |= {(e, float(x)) for x in r[:, 1:].ravel()}
        assert seen == {(e, sg * (k + 0.5)) for e in k8c.TIE_EXPONENTS for k in range(127) for sg in (1, -1)}
        # round-to-nearest-even would give other bytes at every even k
        even = np.floor(np.abs(t[:, 1:].astype(np.float64) / s.astype(np.float64)[:, None])) % 2 == 0
        assert even.sum() >= 2 * 64 * len(k8c.TIE_EXPONENTS)
        # tiny: the subnormal scales, a non-zero row whose scale is 0, and the clamp
        y = fam["tiny"]
        q, s = k8c.quantize_rows(y)
        units = np.rint(y.astype(np.float64) / k8c.U)
        assert np.array_equal(units * k8c.U, y.astype(np.float64)) and np.abs(units).max(-1).tolist() == list(k8c.TINY_N)
        assert s.view(np.uint16).tolist() == [0, 0, 1, 1, 1, 2, 2, 8]
        assert all(n // 2 in np.abs(units[i]) and 1 in np.abs(units[i]) for i, n in enumerate(k8c.TINY_N))
        assert y[:2].any(-1).all() and not q[:2].any(), "scale 0 on a non-zero row: bytes 0"
        i190 = k8c.TINY_N.index(190)
        quot = y[i190].astype(np.float32) / s[i190].astype(np.float32)
        assert np.abs(quot).max() == 190 > 127.5 and np.abs(q[i190].astype(np.int32)).max() == 127, "clamped from 190"
        assert (np.abs(quot) > 127.5).sum() >= 1 and np.abs(q.astype(np.int32)).max() == 127
        # extreme: scale 516, +-258 are exact halves
        x = fam["extreme"]
        q, s = k8c.quantize_rows(x)
        assert x.shape == (1, D) and float(s[0]) == 516.0 and x[0, :4].tolist() == [-65504.0, 258.0, -258.0, 65504.0]
        assert q[0, :4].tolist() == [-127, 1, -1, 127] and q[0, 4:11].tolist() == [2, -3, 4, -5, 6, -7, 8]
        # sweep: the maximum of row c sits at channel c, signs alternate, the D scales are pairwise distinct
        w = fam["sweep"]
        q, s = k8c.quantize_rows(w)
        a = np.abs(w.astype(np.float64))
        c = np.arange(D)
        assert w.shape == (D, D) and np.array_equal(a.argmax(-1), c)
        assert np.array_equal(w[c, c], ((1.0 + c / D) * np.where(c % 2 == 0, 1.0, -1.0)).astype(np.float16))
        a[c, c] = 0
        assert a.max() <= 0.5 and len(set(s.view(np.uint16).tolist())) == D
        assert np.array_equal(q[c, c], np.where(c % 2 == 0, 127, -127))
        q, s = k8c.quantize_rows(fam["zero"])
        assert fam["zero"].shape == (1, D) and s[0] == 0 and not q.any()
        # the identity table
        tab = k8c.identity_table(D, 5)
        assert tab.dtype == np.float16 and tab.shape == (5, D) and (tab[:, : D // 2] == 1).all() and not tab[:, D // 2:].any()
        assert np.array_equal(ac.rope_neox_f16(rows[:, None], tab, np.arange(len(rows)) % 5)[:, 0].view(np.uint16), rows.view(np.uint16))
    assert total <= 300, total


def test_quantised_hot_keys_keep_their_gap():
    """What the GPU hot-row families assert before they launch, at both head widths."""
    for D in (64, 128):
        c = ac.hot_base(2, 4, 300, D, seed=D)
        qc = k8c.quantize_cache(c["k"], c["v"])
        gap = ac.hot_gap(c["q"], qc["kd"], k8c.dequantize_rows(*k8c.quantize_rows(c["hot"])), c["scale"])
        assert gap >= ac.GAP_MIN, gap


# ---- header and library ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_entry_points_are_declared_and_exported(lib):
    from eetq_amd import _lib
    header = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.eetq_abi_version() == 7
    import eetq_amd.ops as ops
    import eetq_amd.ops_ctypes as oc
    for name in ("decode_attention_i8kv", "rope_decode_attention_i8kv", "rotary_embedding_neox_kvcache_prefill_i8"):
        assert name in ops.__all__ and callable(getattr(ops, name)) and name in oc.__all__ and callable(getattr(oc, name))


P = ctypes.c_void_p(1 << 20)     # never dereferenced: every refusal comes before a launch


def _longs(*v):
    return (ctypes.c_long * len(v))(*v)


def _msg(lib):
    return lib.eetq_last_error() or b""


def _decode(lib, D=128, q=P, k=P, v=P, s=P, st=None, sst=None, S=256):
    st = st if st is not None else _longs(4 * D, D, 2 * S * D, S * D, D, 2 * S * D, S * D, D, 0, 4 * D, D)
    sst = sst if sst is not None else _longs(2 * S * 2, S * 2, 2)
    return lib.eetq_decode_attention_i8kv_f16(q, k, v, s, None, P, P, 1, 4, 2, S, D, 1, 0.1, st, sst, None, 0, None, None)


def _rope(lib, D=128, kc=P, vc=P, s=P, st=None, sst=None, S=256, table_rows=64, slot_stride=0):
    st = st if st is not None else _longs(4 * D, 2 * D, 2 * D, 2 * S * D, S * D, D, 2 * S * D, S * D, D, 0, 4 * D, D)
    sst = sst if sst is not None else _longs(2 * S * 2, S * 2, 2)
    return lib.eetq_rope_decode_attention_i8kv_f16(P, None, slot_stride, P, P, P, P, table_rows, kc, vc, s, None, P, P, P, 1, 4, 2, S, D,
                                                   1, 0.1, st, sst, None, 0, None, None)


def _write(lib, D=128, kc=P, vc=P, s=P, st=None, sst=None, S=256, table_rows=64, rot=None, first_row=0, tokens=4, key=P):
    W = 8 * D
    st = st if st is not None else _longs(W, W, W, 2 * S * D, S * D, D)
    sst = sst if sst is not None else _longs(2 * S * 2, S * 2, 2)
    return lib.eetq_rotary_neox_kvcache_prefill_i8_f16(P, P, key, P, P, table_rows, kc, vc, s, 1, tokens, None, first_row, 4, 2, D,
                                                       D if rot is None else rot, st, sst, S, None)


def test_refusals_come_before_any_launch(lib):
    odd = ctypes.c_void_p((1 << 20) + 4)     # 4-byte aligned only
    odd2 = ctypes.c_void_p((1 << 20) + 2)
    for call in (_decode, _rope, _write):
        # head_dim
        assert call(lib, D=96) == ERR_UNSUPPORTED and b"64 and 128" in _msg(lib), call.__name__
        # null pointers
        assert call(lib, s=None) == ERR_INVALID and b"null" in _msg(lib)
        # a cache stride that is no multiple of 8 bytes / a cache that is not 8-byte aligned
        S, D = 256, 128
        bad = {_decode: _longs(4 * D, D, 2 * S * D, S * D, D + 4, 2 * S * D, S * D, D, 0, 4 * D, D),
               _rope: _longs(4 * D, 2 * D, 2 * D, 2 * S * D, S * D, D + 4, 2 * S * D, S * D, D, 0, 4 * D, D),
               _write: _longs(8 * D, 8 * D, 8 * D, 2 * S * D, S * D, D + 4)}[call]
        assert call(lib, st=bad) == ERR_INVALID and b"8 bytes" in _msg(lib)
        kw = {"k": odd} if call is _decode else {"kc": odd}
        assert call(lib, **kw) == ERR_INVALID and b"8-byte aligned" in _msg(lib)
        # the scale row stride a multiple of 2 halfs, the scales 4-byte aligned
        assert call(lib, sst=_longs(2 * S * 3, S * 3, 3)) == ERR_INVALID and b"multiples of 2" in _msg(lib)
        assert call(lib, s=odd2) == ERR_INVALID and b"4-byte aligned" in _msg(lib)
        # the 2 GiB rule, in bytes
        big = 1 << 20
        huge = {_decode: _longs(4 * D, D, 0, 0, big, 0, 0, big, 0, 4 * D, D),
                _rope: _longs(4 * D, 2 * D, 2 * D, 0, 0, big, 0, 0, big, 0, 4 * D, D),
                _write: _longs(8 * D, 8 * D, 8 * D, 0, 0, big)}[call]
        assert call(lib, st=huge) == ERR_INVALID and b"2 GiB" in _msg(lib)
    # fp16 cache rows of the same element count pass the rule in bytes: (256 + 4096) * 2^18 bytes < 2 GiB
    assert _rope(lib, table_rows=0) == ERR_INVALID and b"table" in _msg(lib)
    assert _write(lib, table_rows=0) == ERR_INVALID and b"table" in _msg(lib)
    assert _rope(lib, slot_stride=2) == ERR_INVALID and b"slot_stride" in _msg(lib)
    assert _write(lib, rot=64) == ERR_INVALID and b"rot_dim" in _msg(lib)
    assert _write(lib, first_row=254) == ERR_INVALID and b"inside the cache" in _msg(lib)
    assert _write(lib, key=None) == ERR_INVALID and b"null" in _msg(lib)
    assert _decode(lib, q=ctypes.c_void_p((1 << 20) + 8)) == ERR_INVALID and b"16-byte aligned" in _msg(lib)
    assert _write(lib, tokens=0) == 0          # nothing to do is not an error


# ---- the cache classes -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg():
    transformers = pytest.importorskip("transformers")
    return transformers.LlamaConfig(hidden_size=256, intermediate_size=704, num_hidden_layers=2, num_attention_heads=4,
                                    num_key_value_heads=2, vocab_size=512, max_position_embeddings=128)


def test_int8_static_cache(cfg):
    import torch
    import transformers
    from eetq_amd.utils.kv_cache import Int8StaticCache, Int8StaticLayer
    cache = Int8StaticCache(cfg, max_cache_len=48)
    assert isinstance(cache, transformers.StaticCache) and len(cache.layers) == 2
    assert not cache.layers[0].is_initialized
    cache.allocate(3, "cpu")
    for layer in cache.layers:
        assert isinstance(layer, Int8StaticLayer) and isinstance(layer, transformers.cache_utils.StaticLayer)
        assert layer.is_initialized
        assert layer.keys.shape == layer.values.shape == (3, 2, 48, 64) and layer.keys.dtype == layer.values.dtype == torch.int8
        assert layer.scales.shape == (3, 2, 48, 2) and layer.scales.dtype == torch.float16
        assert layer.get_mask_sizes(1) == (48, 0) and int(layer.get_seq_length()) == 0
        layer.cumulative_length.fill_(7)
        layer.keys.fill_(3)
        layer.scales.fill_(2.0)
    assert int(cache.get_seq_length()) == 7
    cache.reset()
    assert all(int(l.cumulative_length) == 0 and not l.keys.any() and not l.scales.any() for l in cache.layers)
    kv = torch.zeros(3, 2, 1, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="only eet_accelerator attention blocks write an int8 KV cache"):
        cache.update(kv, kv, 0)
    # no fp16 path takes it for a static layer; the int8 path finds it
    from eetq_amd.modules.llama_modules import EETLlamaAttention
    attn = EETLlamaAttention(256, 4, torch.nn.Linear(256, 512), torch.nn.Linear(256, 256), "cpu", num_key_value_heads=2, layer_idx=1,
                             config=cfg)
    assert attn._static_cache_layer(cache) is None
    assert attn._int8_cache_layer(cache) is cache.layers[1]
    assert attn._int8_cache_layer(transformers.StaticCache(config=cfg, max_cache_len=48)) is None
    with pytest.raises(RuntimeError, match="not allocated"):
        attn._int8_cache_layer(Int8StaticCache(cfg, max_cache_len=48))


def test_graph_decoder_refuses_without_a_device(cfg):
    import torch
    import transformers
    from eetq_amd.utils.graph_decoder import GraphDecoder
    for bad in (4, 0, 32, "8", None):
        with pytest.raises(ValueError, match="kv_bits must be 16"):
            GraphDecoder(object(), 2, 32, kv_bits=bad)
    stock = transformers.LlamaForCausalLM(cfg)       # CPU, not accelerated
    with pytest.raises(ValueError, match="kv_bits=8 needs"):
        GraphDecoder(stock, 2, 32, kv_bits=8)
    with pytest.raises(ValueError, match="kv_bits=8 needs"):
        GraphDecoder(torch.nn.Linear(2, 2), 2, 32, kv_bits=8)
