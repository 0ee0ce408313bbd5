"""The library's own static KV caches for the accelerated Llama blocks (extension): int8 rows, and a ring.

``Int8StaticCache`` is a transformers ``StaticCache`` whose layers hold ``keys`` / ``values`` as int8 [B, Hkv, S, D] and one
``scales`` tensor, float16 [B, Hkv, S, 2] = (k scale, v scale) of each row: ``2 D + 4`` bytes per row against ``4 D``.  Rows are
written and read by the library's own kernels only (``ops.rotary_embedding_neox_kvcache_prefill_i8``,
``ops.rope_decode_attention_i8kv``, ``ops.decode_attention_i8kv``), which the ``eet_accelerator`` attention blocks call when they
meet such a layer; the stock ``update()`` path refuses it.  ``GraphDecoder(..., kv_bits=8)`` builds one.

``RollingStaticCache`` is a ``StaticCache`` of fp16 rows whose layers hold ``ring_rows(window, chunk)`` rows instead of the
sequence's length: under ``llama_modules.sliding_window_static(window, ring=True)`` the attention blocks write logical row r at
row ``r mod R`` and attend through the ring forms of the windowed kernels, so a cache of about ``window`` rows serves a sequence
of any length.  ``GraphDecoder(..., window=W, rolling=True)`` builds one.
"""
import torch
from transformers.cache_utils import Cache, StaticCache, StaticLayer

__all__ = ["Int8StaticLayer", "Int8StaticCache", "RollingStaticCache", "ring_rows"]


def ring_rows(window, chunk):
    """The rows R of a ring cache that serves a sliding window of ``window`` rows with prompt pieces of at most ``chunk`` rows: the
    least multiple of 64 with ``R >= window + chunk + 62`` (pure function).  The prompt kernel reads whole 64-row key blocks, the
    lowest of them starting up to 62 rows below a piece's first window, and must not meet the rows the piece's own cache write has
    just replaced; a multiple of 64 keeps a key block from straddling the ring's end.  A decode step needs ``R >= window`` only."""
    for name, v in (("window", window), ("chunk", chunk)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError("ring_rows: %s must be an integer of at least 1 row, got %r" % (name, v))
    return 64 * ((window + chunk + 62 + 63) // 64)


class Int8StaticLayer(StaticLayer):
    """One layer of an ``Int8StaticCache``.  Allocated eagerly (``allocate``): there is no float key to learn a dtype from.
    ``cumulative_length``, ``get_mask_sizes``, ``get_seq_length`` and ``reset`` are the static layer's."""

    supports_early_init = False

    def __init__(self, max_cache_len, **kwargs):
        super().__init__(max_cache_len=max_cache_len)
        self.scales = None

    def allocate(self, batch, heads, head_dim, device):
        self.dtype, self.device = torch.int8, torch.device(device)
        self.batch_size, self.num_heads = int(batch), int(heads)
        self.k_head_dim = self.v_head_dim = int(head_dim)
        shape = (self.batch_size, self.num_heads, self.max_cache_len, self.k_head_dim)
        self.keys = torch.zeros(shape, dtype=torch.int8, device=self.device)
        self.values = torch.zeros(shape, dtype=torch.int8, device=self.device)
        self.scales = torch.zeros(shape[:3] + (2,), dtype=torch.float16, device=self.device)
        self.cumulative_length = self.cumulative_length.to(self.device)
        self.is_initialized = True
        return self

    def lazy_initialization(self, key_states, value_states):
        raise RuntimeError("Int8StaticLayer is allocated eagerly: call allocate(batch, heads, head_dim, device)")

    def update(self, key_states, value_states, *args, **kwargs):
        raise RuntimeError("Int8StaticLayer.update: only eet_accelerator attention blocks write an int8 KV cache (its rows are "
                           "quantised by the library's kernels); this attention block called the stock cache update")

    def reset(self):
        super().reset()
        if self.scales is not None:
            self.scales.zero_()


class Int8StaticCache(StaticCache):
    """``StaticCache`` with int8 rows and per-row scales: one ``Int8StaticLayer`` per decoder layer (full attention only)."""

    def __init__(self, config, max_cache_len, **kwargs):
        text = config.get_text_config(decoder=True) if hasattr(config, "get_text_config") else config
        kinds = getattr(text, "layer_types", None)
        if kinds is not None and any(k != "full_attention" for k in kinds):
            raise ValueError("Int8StaticCache: full-attention layers only (got layer_types=%r)" % (kinds,))
        self._text_config = text
        Cache.__init__(self, layers=[Int8StaticLayer(max_cache_len) for _ in range(text.num_hidden_layers)])

    def allocate(self, batch, device):
        """Allocate every layer for ``batch`` rows on ``device`` (shapes from the model config)."""
        text = self._text_config
        heads = getattr(text, "num_key_value_heads", None) or text.num_attention_heads
        head_dim = getattr(text, "head_dim", None) or text.hidden_size // text.num_attention_heads
        for layer in self.layers:
            layer.allocate(batch, heads, head_dim, device)
        return self


class RollingStaticCache(StaticCache):
    """``StaticCache`` whose layers are rings of ``ring_rows(window, chunk)`` fp16 rows (full attention only): plain ``StaticLayer``s,
    allocated as zeros by the first forward like any static cache -- a ring must hold finite values everywhere, and its stale rows
    are old real rows --, each with its device token counter, which keeps counting the sequence's tokens (it is the logical length
    the ring kernels take; it is not bounded by the rows).  Only attention blocks that run under
    ``llama_modules.sliding_window_static(window, ring=True)`` address it correctly: the stock ``update()`` path would write
    beyond row R."""

    def __init__(self, config, window, chunk, **kwargs):
        text = config.get_text_config(decoder=True) if hasattr(config, "get_text_config") else config
        kinds = getattr(text, "layer_types", None)
        if kinds is not None and any(k != "full_attention" for k in kinds):
            raise ValueError("RollingStaticCache: full-attention layers only (got layer_types=%r)" % (kinds,))
        self.window, self.chunk = window, chunk
        self.ring_rows = ring_rows(window, chunk)
        super().__init__(config=config, max_cache_len=self.ring_rows, **kwargs)
