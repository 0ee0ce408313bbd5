"""Greedy decode with a static KV cache and captured HIP graphs: one replay per generated token, or per several.

The reference's end-to-end recipe (examples/models/llama_transformers_example.py:68-79) calls transformers'
``generate``; with ~360 short kernels per token at Llama-13B shapes that loop is bound by host launch time, not by the
GPU.  The decode step is launch-bound inner-loop work, so it is captured once (token id and position live in static device
tensors; the static cache's own token counter is advanced on the device by the attention kernel) and replayed per token.
Prefill stays eager.  Works with any transformers causal LM whose forward accepts ``past_key_values`` / ``cache_position``
(stock Llama, ``eet_quantize``-d or ``eet_accelerator``-ed).
"""
import contextlib
import inspect

import torch

__all__ = ["GraphDecoder", "left_pad_starts"]


def left_pad_starts(mask):
    """The first real column of every row of a LEFT-padded batch: ``mask`` [B, P] holds keep flags (bool or integer, non-zero =
    a real token), as a tokenizer with ``padding_side="left"`` returns them; the result is ``P - mask.sum(1)``, int64 [B] on the
    mask's device.  A row with a hole, right padding or no real token at all raises ``ValueError``, and so does a mask that is
    not 2-D.  One host read."""
    mask = torch.as_tensor(mask)
    if mask.dim() != 2 or mask.shape[1] < 1:
        raise ValueError("GraphDecoder: attention_mask must be [batch, P] keep flags, got shape %s" % (tuple(mask.shape),))
    if mask.is_floating_point() or mask.is_complex():
        raise ValueError("GraphDecoder: attention_mask must hold bool or integer keep flags, got %s" % (mask.dtype,))
    keep = mask != 0
    P = keep.shape[1]
    starts = P - keep.sum(1, dtype=torch.int64)
    left_padded = keep == (torch.arange(P, device=keep.device)[None, :] >= starts[:, None])
    ok, some = torch.stack([left_padded.all(), (starts < P).all()]).tolist()
    if not some:
        raise ValueError("GraphDecoder: every row of attention_mask must keep at least one token")
    if not ok:
        raise ValueError("GraphDecoder: attention_mask must be left-padded (zeros, then ones, in every row): a row has a hole or "
                         "padding on the right")
    return starts


def _lean_model(model, lean):
    """``GraphDecoder._lean`` of a decoder that is not built yet."""
    base = getattr(model, "model", None)
    layers = getattr(base, "layers", None)
    return bool(lean and layers is not None and len(layers) > 0 and hasattr(base, "embed_tokens") and hasattr(base, "norm")
                and hasattr(model, "lm_head") and all(getattr(l, "fused_layer_step", False) for l in layers))


def _require_accelerated(setting, model, lean, prompt_kernel):
    """What ``ragged``, ``kv_bits=8``, ``window`` and ``speculative`` need of the model (``setting``: the one that asks, as the caller
    wrote it): the lean layer loop over accelerated layers -- their attention blocks alone take a per-row first key, a window, a
    device length or int8 rows -- at the head sizes their kernels have; with ``prompt_kernel`` the MFMA prompt kernel as well, the
    only prompt path with a window or a device length."""
    if not _lean_model(model, lean):
        raise ValueError("GraphDecoder: %s needs lean=True and a fully accelerated model (eet_accelerator with fused_attn, "
                         "fused_mlp and fused_residual): only its attention blocks run what the setting asks for" % setting)
    from .. import ops
    for layer in model.model.layers:
        attn = getattr(layer, "self_attn", None)
        if not hasattr(attn, "decode_step_state") or getattr(attn, "head_dim", None) not in (64, 128):
            raise ValueError("GraphDecoder: %s needs attention blocks with head size 64 or 128" % setting)
        if prompt_kernel and (not getattr(attn, "mfma_prefill", False) or not getattr(attn, "static_prefill", False)
                              or ops.prefill_attention is None or not ops.prefill_attention_supported(attn.head_dim)):
            raise ValueError("GraphDecoder: %s needs the MFMA prompt kernel (the compiled operator module, mfma_prefill=True, "
                             "static_prefill=True): no other prompt path runs what the setting asks for" % setting)


class GraphDecoder:
    def __init__(self, model, batch, max_len, capture=True, lean=True, steps_per_graph=7, sampling=False, kv_bits=16, kv8_append=False,
                 ragged=False, speculative=0, ngram=3, draft=None, spec_sampling=False, spec_attention="prompt", window=None,
                 rolling=False, rolling_chunk=512):
        """``max_len``: cache rows (prompt + new tokens).  ``capture=False`` keeps the same static-cache stepping but runs
        every step eagerly (used to check the graph against the launches it was captured from).  ``lean``: step fully
        accelerated models layer by layer instead of through the stock model forward (see ``_lean``).
        ``steps_per_graph``: a second graph holds that many consecutive steps (one replay = that many tokens); the token
        hand-over between steps (next input id, position, the output row) is done by launches INSIDE the graphs, so a
        generated token costs the host one ``replay`` per ``steps_per_graph`` tokens and nothing else -- with one graph
        per token plus three eager bookkeeping launches the host side was 0.125 ms of every 2.96 ms token at 13B shapes
        (``profiles/r06_bench_*.json``: decode_budget.step_us vs the end-to-end time).
        ``sampling``: the hand-over inside the graphs is ``ops.sample_handover`` on a static parameter block and static EOS
        flags instead of the argmax: ``generate`` then takes ``do_sample`` / ``temperature`` / ``top_k`` / ``top_p`` / ``seed`` /
        ``eos_token_id`` / ``pad_token_id`` per call, without recapture (needs fp16 logits on the GPU).  The default leaves
        launches and tokens as they were.
        ``kv_bits``: 16 (the default: an fp16 ``StaticCache``) or 8: an ``Int8StaticCache`` (``utils/kv_cache.py``: int8 rows with a
        scale pair each, ``2 D + 4`` bytes per row against ``4 D``), written and read by the accelerated attention blocks' int8
        kernels.  It needs the lean layer-by-layer model with head size 64 or 128, and by default runs fresh whole prompts only:
        ``append=True`` and chunked prompts raise ``ValueError``.
        ``kv8_append`` (``kv_bits=8`` only; default ``False``): the opt-in for ``append=True``, ``prefill_chunk=`` and
        ``prefill(chunk=, append=)`` on the int8 cache, and the acceptance of what they mean there: a piece behind cached rows
        writes its rows first and then attends the DEQUANTISED rows 0 .. counter - 1 (``ops.prefill_attention_i8kv``), its own keys
        and values as their quantised selves, as a decode step does.  A chunked prompt is therefore NOT bit-identical to the
        whole prompt on an int8 cache: the first piece of an emptied cache stays on the fresh path (unquantised keys, the fp16
        decoder's bits), later pieces see quantised earlier rows.  The captured decode graphs are reused as they
        are after an append.
        ``ragged`` (default ``False``: nothing changes): the decoder takes LEFT-padded batches -- ``generate`` and ``prefill`` accept
        ``attention_mask`` [batch, P] keep flags.  It owns a static ``s_start`` [batch] (each row's first real cache row), captures
        its graphs under ``llama_modules.padded_static_batch(s_start)`` -- the attention kernels then count every row's blocks from
        its first real token and never read its pad rows -- and steps with ``position_ids = s_pos - s_start`` (one small launch per
        step, inside the graph); ``s_pos`` remains the cache row.  The decode step goes through the attention module instead of
        the one-call layer.  It needs the lean layer-by-layer model with head size 64 or 128 and an fp16 cache (``kv_bits=16``).
        ``speculative`` (default 0: nothing changes, no state, the same graphs): ``k`` in 1 .. 15 builds a speculative greedy
        decoder.  One verify step drafts ``k`` tokens, runs the model once over the ``k + 1`` rows
        [pending token | draft] behind the cached rows (``appended_static_prefill``: the attention blocks write rows counter ..
        counter + k and attend through the device counter), and ``ops.spec_accept`` hands over the 1 .. k + 1 tokens every batch
        row confirms; the rejected rows are rolled back by setting the cache counters to the position (rows at or beyond the
        counter are never read).  The emitted tokens are those of greedy decoding up to the kernels' rounding: a verify pass
        computes a token's logits with the prompt kernels, a plain step with the decode kernels.  The step is its own captured
        graph; the plain graphs are captured too and serve ``generate(speculate=False)``.  It needs what ``ragged`` needs --
        ``lean``, a fully accelerated model, head size 64 or 128, ``kv_bits=16`` -- and the MFMA prompt kernel; ``ragged``,
        ``sampling`` (without ``spec_sampling``, below) and ``kv_bits=8`` (without ``kv8_append``, next) raise ``ValueError``.
        ``generate`` then needs ``k`` spare cache rows.
        On an INT8 cache (``kv_bits=8``) a verify pass is rows appended behind quantised rows, so ``kv8_append=True`` -- the existing
        acceptance of exactly that -- is what lets ``speculative=k`` build there: the verify step runs under
        ``appended_static_prefill(int8_rows=True)``, writes its ``k + 1`` rows quantised behind the device counter and attends the
        DEQUANTISED rows through ``ops.prefill_attention_i8kv`` (or, with ``spec_attention="rows"``, the few-row kernel's int8-row
        form).  Draft, accept, history, stats, the spare rows and the one-copy rollback are the fp16 decoder's: stale bytes and
        scales behind the counter are never read.  Without ``kv8_append`` the combination keeps raising.
        ``ngram`` (1 .. 8): the longest n-gram ``ops.ngram_draft`` looks up in the sequence's own history (``s_hist``).
        ``draft``: a callable ``draft(decoder) -> [batch, k]`` int64 tokens on the device (valid vocabulary ids) instead of the
        lookup: the hook for a draft model and for tests.  Under capture its launches are what the graph holds: it is called
        while capturing, never per step, so it must read and write static tensors only (``s_hist``, ``s_pos``, ``s_tok`` ...)
        and read nothing on the host.  It stays a POINT-MASS draft: tokens, not distributions.
        ``spec_sampling`` (default ``False``: nothing changes): the opt-in for ``speculative=k`` together with ``sampling=True``
        (DESIGN.md 4.17); it needs both.  The verify step then hands over through ``ops.spec_sample_accept`` on the static
        parameter block, the EOS flags and a static workspace: every verify row's token is drawn as ``ops.sample_handover`` draws
        it at that token's own output column, a draft token is accepted iff it IS the drawn token -- exact speculative sampling
        for a point-mass draft -- and a finished row hands on the pad token and never ends a step.  ``generate`` takes the
        sampling and EOS arguments of a ``sampling=True`` decoder.  For one seed the speculative and the plain sampled decoder
        compute the SAME function of the logits (token c of row b from its prefix's logits and Philox(seed; c, b)): their outputs
        differ only where the prompt kernels of a verify pass and the decode kernels of a plain step round a logit differently.
        ``generate(speculate=False)`` replays the plain sampling graphs.
        ``spec_attention`` (default ``"prompt"``: the verify step as it has always been captured, bit for bit): ``"rows"`` runs the
        verify step's layers under ``appended_static_prefill(few_rows=True)``, so the attention of its ``k + 1`` rows is
        ``ops.decode_attention_rows`` -- the split-KV MFMA kernel for a few rows behind a long cache -- instead of
        the prompt kernel, under greedy and under ``spec_sampling=True`` verification alike.  It needs ``speculative=k`` and the
        compiled operator module; any other value raises ``ValueError``.  ``prefill`` and ``generate(append=True)`` keep the
        prompt kernel.  On an int8 speculative decoder (``kv_bits=8, kv8_append=True``) ``"rows"`` is
        ``appended_static_prefill(int8_rows=True, few_rows_int8=True)`` and ``ops.decode_attention_rows_i8kv`` (the
        chunk rule is the fp16 rows' and untuned for int8 rows); ``"prompt"`` stays the default there as well.
        ``window`` (default ``None``: nothing changes): an integer ``W >= 1`` builds a SLIDING-WINDOW decoder: every
        forward, captured or eager, runs under ``llama_modules.sliding_window_static(W)``, so a token at cache row p attends rows
        ``max(0, p - W + 1) .. p`` -- prompts through the windowed MFMA prompt kernel, steps through the windowed decode kernels,
        the window a kernel argument of the captured graphs.  The cache stays the static ``max_len``-row cache (rows are not
        recycled); ``generate``, ``prefill(chunk=)``, ``append=True`` and sampling work as without it.  The decode step goes through
        the attention module instead of the one-call layer.  It needs what ``ragged`` needs -- ``lean``, a fully accelerated model,
        head size 64 or 128 -- and the MFMA prompt kernel; ``ragged=True`` (no ragged prompt with a window), ``kv_bits=8`` (no window
        on int8 rows) and ``speculative=k`` (the verify step's kernels have no window) raise ``ValueError``.
        ``rolling`` (default ``False``; needs ``window``): the cache becomes a ``kv_cache.RollingStaticCache`` -- a RING of
        ``kv_cache.ring_rows(W, rolling_chunk)`` rows per layer instead of ``max_len`` -- and every forward runs under
        ``sliding_window_static(W, ring=True)``.  ``max_len`` stays the bound on the SEQUENCE: the token buffers and the rotary table
        cover it, the cache does not.  ``generate`` / ``prefill`` cut any prompt into pieces of at most ``rolling_chunk`` tokens (a
        smaller ``prefill_chunk`` / ``chunk`` is kept), the first fresh, the later ones appended; ``append=True``, sampling, captured and
        eager stepping work as without it, and one captured graph serves every length: wrapping is kernel arithmetic on the device
        counter.  ``rolling=True`` without ``window``, or with ``ragged``, ``kv_bits=8`` or ``speculative``, raises ``ValueError``."""
        self.window = self._check_window(window, model, lean, ragged, kv_bits, speculative)
        self.rolling, self.rolling_chunk = self._check_rolling(rolling, rolling_chunk, window, ragged, kv_bits, speculative)
        if spec_attention not in ("prompt", "rows"):
            raise ValueError("GraphDecoder: spec_attention must be 'prompt' (the MFMA prompt kernel) or 'rows' (the few-row split-KV "
                             "kernel), got %r" % (spec_attention,))
        if spec_attention == "rows":
            from .. import ops as _ops
            if not speculative:
                raise ValueError("GraphDecoder: spec_attention='rows' chooses the attention of the verify step and needs a "
                                 "speculative decoder (speculative=k)")
            if _ops.decode_attention_rows is None:
                raise ValueError("GraphDecoder: spec_attention='rows' needs ops.decode_attention_rows, which lives in the compiled "
                                 "operator module (this process runs the ctypes boundary)")
            if kv_bits == 8 and _ops.decode_attention_rows_i8kv is None:
                raise ValueError("GraphDecoder: spec_attention='rows' on an int8 cache needs ops.decode_attention_rows_i8kv, which "
                                 "lives in the compiled operator module")
        self.spec_attention = spec_attention
        if kv_bits not in (8, 16):
            raise ValueError("GraphDecoder: kv_bits must be 16 (fp16 cache) or 8 (int8 cache), got %r" % (kv_bits,))
        if kv8_append and kv_bits != 8:
            raise ValueError("GraphDecoder: kv8_append=True is the opt-in of an int8 cache (kv_bits=8), got kv_bits=%r" % (kv_bits,))
        self.kv_bits = int(kv_bits)
        self.kv8_append = bool(kv8_append)
        self.lean = bool(lean)
        self.sampling = bool(sampling)
        self.model = model
        self.ragged = bool(ragged)
        if not isinstance(spec_sampling, bool):
            raise ValueError("GraphDecoder: spec_sampling must be True or False, got %r" % (spec_sampling,))
        if spec_sampling and not (self.sampling and speculative):
            raise ValueError("GraphDecoder: spec_sampling=True is the opt-in for speculative=k together with sampling=True and "
                             "needs both, got speculative=%r, sampling=%r" % (speculative, sampling))
        self.speculative = self._check_speculative(speculative, ngram, draft, max_len, spec_sampling)
        self.ngram = int(ngram)
        self._draft_fn = draft
        if self.ragged:
            if self.kv_bits != 16:
                raise ValueError("GraphDecoder: ragged=True needs an fp16 cache (kv_bits=16): the int8 kernels take no per-row first "
                                 "key, got kv_bits=%r" % (kv_bits,))
            _require_accelerated("ragged=True", model, lean, prompt_kernel=False)
        if self.kv_bits == 8:
            _require_accelerated("kv_bits=8", model, lean, prompt_kernel=False)
        from transformers import StaticCache
        self.batch = int(batch)
        self.max_len = int(max_len)
        dev = next(model.parameters()).device
        self.device = dev
        if self.kv_bits == 8:
            from .kv_cache import Int8StaticCache
            self.cache = Int8StaticCache(config=model.config, max_cache_len=self.max_len).allocate(self.batch, dev)
        elif self.rolling:
            from .kv_cache import RollingStaticCache
            self.cache = RollingStaticCache(config=model.config, window=self.window, chunk=self.rolling_chunk)
            # the rotary tables cover the sequence, not the ring (grown here: never during capture)
            for layer in model.model.layers:
                layer.self_attn._grow_table(self.max_len)
        else:
            try:
                self.cache = StaticCache(config=model.config, max_cache_len=self.max_len)
            except TypeError:  # older constructor
                self.cache = StaticCache(config=model.config, max_batch_size=self.batch, max_cache_len=self.max_len, device=dev,
                                         dtype=torch.float16)
        self.s_tok = torch.zeros(self.batch, 1, dtype=torch.long, device=dev)
        self.s_pos = torch.zeros(1, dtype=torch.long, device=dev)
        # ragged: every row's first real cache row (the kernels' kv_start; the captured graphs read this very tensor)
        self.s_start = torch.zeros(self.batch, dtype=torch.long, device=dev) if self.ragged else None
        # generated tokens: step i of a generate() writes column s_idx (a device counter the graphs advance themselves)
        self.s_idx = torch.zeros(1, 1, dtype=torch.long, device=dev)
        self.out_buf = torch.zeros(self.batch, self.max_len + 1, dtype=torch.long, device=dev)
        self.params = self.done = None
        if self.sampling:
            from ..sampling import sampling_params
            self.params = sampling_params(temperature=0.0, device=dev)
            self.done = torch.zeros(self.batch, dtype=torch.int32, device=dev)   # per row: EOS drawn (readable after generate)
        self.graph = None
        self.graph_n = None
        self.graph_spec = None
        if self.speculative:
            k = self.speculative
            # the rows' tokens by cache row (column position = the pending token), the step's draft, the output column generate
            # stops at, (verify steps, tokens) of the current generate
            self.s_hist = torch.zeros(self.batch, self.max_len, dtype=torch.long, device=dev)
            self.s_draft = torch.zeros(self.batch, k, dtype=torch.long, device=dev)
            self.s_limit = torch.zeros(1, dtype=torch.long, device=dev)
            self.s_stats = torch.zeros(2, dtype=torch.long, device=dev)
            self._spec_offsets = torch.arange(k + 1, dtype=torch.long, device=dev)
            if spec_sampling:   # the verify rows' tokens between their workgroups and the one that hands over
                self.spec_sampling = True
                self.s_spec_ws = torch.zeros(self.batch * (k + 1), dtype=torch.long, device=dev)
        # the prompt pass needs the LAST position's logits only (the stock forward projects all of them onto the vocabulary)
        params = inspect.signature(model.forward).parameters
        self._last_logits_only = {"logits_to_keep": 1} if "logits_to_keep" in params else {}
        self.steps_per_graph = max(1, int(steps_per_graph))
        with torch.no_grad():
            # the cache tensors are allocated lazily by the first forward: run one tiny prefill before capturing
            first = model(self.s_tok, past_key_values=self.cache, cache_position=self.s_pos, use_cache=True)
            if self.sampling and not (first.logits.is_cuda and first.logits.dtype == torch.float16):
                raise ValueError("GraphDecoder: sampling=True needs float16 logits on the GPU (got %s on %s)"
                                 % (first.logits.dtype, first.logits.device))
            if capture:
                with self._promise():   # (the allocating forward above ran without it: no cache layer, nothing to promise yet)
                    self._capture()
                if self.speculative:
                    self._capture_spec()
        self.cache.reset()
        # host-side bookkeeping of a conversation: cache rows written, and whether s_tok holds a token the caller has seen but the
        # cache has not (the last one a generate() emitted)
        self.rows = 0
        self._pending = False

    def _capture(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._advance()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._advance()
        if self.steps_per_graph > 1:
            self.graph_n = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_n):
                for _ in range(self.steps_per_graph):
                    self._advance()

    @staticmethod
    def _check_window(window, model, lean, ragged, kv_bits, speculative):
        """The checked ``window`` (``None``: off).  Every refusal says which setting and why."""
        if window is None:
            return None
        if isinstance(window, bool) or not isinstance(window, int) or window < 1:
            raise ValueError("GraphDecoder: window must be None (off) or the sliding window's rows, an integer >= 1, got %r" % (window,))
        if ragged:
            raise ValueError("GraphDecoder: window=%d with ragged=True: the windowed prompt kernel knows one shared first key only "
                             "(ragged prompts with a window are not built)" % window)
        if kv_bits != 16:
            raise ValueError("GraphDecoder: window=%d needs an fp16 cache (kv_bits=16): the int8 kernels have no sliding window, got "
                             "kv_bits=%r" % (window, kv_bits))
        if speculative:
            raise ValueError("GraphDecoder: window=%d with speculative=%r: the verify step attends k + 1 rows behind the cache with "
                             "kernels that have no sliding window" % (window, speculative))
        _require_accelerated("window=%d" % window, model, lean, prompt_kernel=True)
        return int(window)

    @staticmethod
    def _check_rolling(rolling, rolling_chunk, window, ragged, kv_bits, speculative):
        """The checked (``rolling``, ``rolling_chunk``).  Every refusal says which setting and why."""
        if not rolling:
            return False, None
        if window is None:
            raise ValueError("GraphDecoder: rolling=True needs window=W: a rolling cache holds the last rows of a sliding window only")
        if ragged:
            raise ValueError("GraphDecoder: rolling=True with ragged=True: there is no ragged ring (the ring kernels know one shared "
                             "first key)")
        if kv_bits != 16:
            raise ValueError("GraphDecoder: rolling=True needs an fp16 cache (kv_bits=16): there is no ring of int8 rows, got "
                             "kv_bits=%r" % (kv_bits,))
        if speculative:
            raise ValueError("GraphDecoder: rolling=True with speculative=%r: the verify step's kernels read cache rows by their "
                             "logical index (no ring)" % (speculative,))
        if isinstance(rolling_chunk, bool) or not isinstance(rolling_chunk, int) or rolling_chunk < 1:
            raise ValueError("GraphDecoder: rolling_chunk must be the longest prompt piece, an integer >= 1, got %r" % (rolling_chunk,))
        return True, int(rolling_chunk)

    def _check_speculative(self, speculative, ngram, draft, max_len, spec_sampling=False):
        """The checked ``speculative`` (0: off).  Every refusal says which setting and why."""
        if isinstance(speculative, bool) or not isinstance(speculative, int) or not 0 <= speculative <= 15:
            raise ValueError("GraphDecoder: speculative must be 0 (off) or the draft length, 1 .. 15, got %r" % (speculative,))
        if not speculative:
            if draft is not None:
                raise ValueError("GraphDecoder: draft= is the draft of a speculative decoder (speculative=k)")
            return 0
        if isinstance(ngram, bool) or not isinstance(ngram, int) or not 1 <= ngram <= 8:
            raise ValueError("GraphDecoder: ngram must lie in 1 .. 8, got %r" % (ngram,))
        if draft is not None and not callable(draft):
            raise ValueError("GraphDecoder: draft must be a callable draft(decoder) -> [batch, k] int64 tokens on the device")
        if self.sampling and not spec_sampling:
            raise ValueError("GraphDecoder: speculative=%d does greedy verification only: a draft token is accepted when it IS the "
                             "argmax, which says nothing about a sampled token (sampling=True); spec_sampling=True opts in to the "
                             "sampled verify step, which accepts a draft token when it IS the drawn token" % speculative)
        if self.ragged:
            raise ValueError("GraphDecoder: speculative=%d advances all rows by one shared cache counter and one position; "
                             "ragged=True steps every row from its own first key" % speculative)
        if self.kv_bits != 16 and not self.kv8_append:
            raise ValueError("GraphDecoder: speculative=%d needs fp16 cache rows (kv_bits=16): the verify pass attends behind the "
                             "device counter with the fp16 prompt kernel, got kv_bits=%r; on an int8 cache kv8_append=True opts in "
                             "to a verify pass that attends the quantised rows (its own among them)"
                             % (speculative, self.kv_bits))
        # (the verify pass is the lean layer loop over k + 1 rows, attended through the device counter)
        _require_accelerated("speculative=%d" % speculative, self.model, self.lean, prompt_kernel=True)
        if int(max_len) < speculative + 1:
            raise ValueError("GraphDecoder: speculative=%d writes %d cache rows per verify step, the cache has %d"
                             % (speculative, speculative + 1, int(max_len)))
        return int(speculative)

    def _capture_spec(self):
        """Warm the verify step up and capture it.  With ``s_limit`` = 0 a step hands over nothing and rolls back to row 0."""
        counters = [layer.cumulative_length for layer in self.cache.layers]
        torch._foreach_zero_(counters)
        self.s_pos.zero_()
        self.s_idx.zero_()
        self.s_limit.zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._advance_spec()
        torch.cuda.current_stream().wait_stream(side)
        self.graph_spec = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_spec):
            self._advance_spec()
        self.s_stats.zero_()

    def _promise(self):
        """``padded_static_batch(s_start)`` on a ragged decoder, ``sliding_window_static(window)`` on a windowed one (every forward,
        captured or eager, runs inside it), else nothing."""
        if self.window is not None:
            from ..modules.llama_modules import sliding_window_static
            return sliding_window_static(self.window, ring=self.rolling)
        if not self.ragged:
            return contextlib.nullcontext()
        from ..modules.llama_modules import padded_static_batch
        return padded_static_batch(self.s_start)

    def _fresh_prefill_ok(self):
        """True when the prompt may run under ``fresh_static_prefill``: the lean layer-by-layer model, every attention block
        able to take its static-cache prompt path (initialised cache layer, supported head size)."""
        if not self._lean():
            return False
        for layer in self.model.model.layers:
            attn = getattr(layer, "self_attn", None)
            if attn is None or not getattr(attn, "static_prefill", False) or not hasattr(attn, "_static_cache_layer"):
                return False
            if attn._static_cache_layer(self.cache) is None and (not hasattr(attn, "_int8_cache_layer")
                                                                 or attn._int8_cache_layer(self.cache) is None):
                return False
        return True

    def _lean(self):
        """True when every decoder layer is an accelerated one (eet_accelerator with fused_attn / fused_mlp / fused_residual):
        those read positions and the cache's own token counter and need neither the causal mask nor the cos / sin tensors
        the stock ``LlamaModel.forward`` builds on every step (~20 small launches per token)."""
        return _lean_model(self.model, self.lean)

    def _logits(self):
        """The last position's logits [batch, vocab] of one decode step on the static tensors."""
        if self._lean():
            base = self.model.model
            h = base.embed_tokens(self.s_tok)
            if self.ragged:   # a row's position counts from its first real token; s_pos is the cache row
                pos = (self.s_pos - self.s_start).view(self.batch, 1)
            else:
                pos = self.s_pos.view(1, 1).expand(self.batch, 1)
            for layer in base.layers:
                h = layer(h, attention_mask=None, position_ids=pos, past_key_values=self.cache, use_cache=True)
                if isinstance(h, tuple):
                    h = h[0]
            lg = self.model.lm_head(base.norm(h))
        else:
            lg = self.model(self.s_tok, past_key_values=self.cache, cache_position=self.s_pos, use_cache=True).logits
        return lg[:, -1]

    def _step(self):
        return self._logits().argmax(-1, keepdim=True)

    def _advance(self):
        """One step and its hand-over, all on the device: the new token goes to its output column and becomes the next
        input id; position and output column move on -- one library launch (``ops.greedy_handover``: torch.argmax's answer)
        where the logits are fp16 on the GPU, otherwise argmax + scatter_ + copy_ + two add_."""
        lg = self._logits()
        if self.sampling:
            from .. import ops
            ops.sample_handover(lg if lg.stride(-1) == 1 else lg.contiguous(), self.out_buf, self.s_idx, self.s_tok, self.s_pos,
                                self.params, self.done)
            return
        if lg.is_cuda and lg.dtype == torch.float16 and lg.stride(-1) == 1:
            from .. import ops
            ops.greedy_handover(lg, self.out_buf, self.s_idx, self.s_tok, self.s_pos)
            return
        nxt = lg.argmax(-1, keepdim=True)
        self.out_buf.scatter_(1, self.s_idx.expand(self.batch, 1), nxt)
        self.s_tok.copy_(nxt)
        self.s_pos.add_(1)
        self.s_idx.add_(1)

    def _advance_spec(self):
        """One verify step, all on the device: draft, the model over the k + 1 rows [pending token | draft] behind the cached
        rows, accept + hand-over of 1 .. k + 1 tokens, and the rollback of the rejected rows (counter = position)."""
        from .. import ops
        from ..modules.llama_modules import appended_static_prefill
        k = self.speculative
        if self._draft_fn is not None:
            d = self._draft_fn(self)
            if (not torch.is_tensor(d) or tuple(d.shape) != (self.batch, k) or d.dtype != torch.long or d.device != self.s_draft.device):
                raise ValueError("GraphDecoder: draft(decoder) must return [batch, k] = [%d, %d] int64 tokens on the device"
                                 % (self.batch, k))
            if d is not self.s_draft:
                self.s_draft.copy_(d)
        else:
            ops.ngram_draft(self.s_hist, self.s_pos, self.s_draft, self.ngram)
        base = self.model.model
        ids = torch.cat([self.s_tok, self.s_draft], dim=1)                                    # [B, k + 1]
        pos = (self.s_pos + self._spec_offsets).view(1, k + 1).expand(self.batch, k + 1)      # cache rows = positions
        h = base.embed_tokens(ids)
        rows_kernel = self.spec_attention == "rows"
        if self.kv_bits == 8:   # (kv8_append: _check_speculative) the verify rows attend quantised rows, their own among them
            ctx = appended_static_prefill(int8_rows=True, few_rows_int8=rows_kernel)
        else:
            ctx = appended_static_prefill(few_rows=rows_kernel)
        with ctx:
            for layer in base.layers:
                h = layer(h, attention_mask=None, position_ids=pos, past_key_values=self.cache, use_cache=True)
                if isinstance(h, tuple):
                    h = h[0]
        lg = self.model.lm_head(base.norm(h))
        if not (lg.is_cuda and lg.dtype == torch.float16):
            raise ValueError("GraphDecoder: speculative decoding needs float16 logits on the GPU (got %s on %s)" % (lg.dtype, lg.device))
        if getattr(self, "spec_sampling", False):
            ops.spec_sample_accept(lg if lg.stride(-1) == 1 else lg.contiguous(), self.s_draft, self.out_buf, self.s_idx, self.s_tok,
                                   self.s_pos, self.s_limit, self.s_hist, self.s_stats, self.params, self.done, None, self.s_spec_ws)
        else:
            ops.spec_accept(lg if lg.stride(-1) == 1 else lg.contiguous(), self.s_draft, self.out_buf, self.s_idx, self.s_tok, self.s_pos,
                            self.s_limit, self.s_hist, self.s_stats)
        # the rollback: the blocks advanced their counters by k + 1; rows at or beyond the position were rejected (or hold the
        # new pending token's predecessors' drafts) and are never read once the counter says so -- one launch for all layers
        counters = [layer.cumulative_length for layer in self.cache.layers]
        torch._foreach_copy_(counters, [self.s_pos.view(c.shape) for c in counters])

    def spec_stats(self):
        """(verify steps, tokens they handed over) of the last ``generate`` on a speculative decoder -- the first token, which
        comes from the prompt's logits, is not among them.  One host read."""
        if not self.speculative:
            raise ValueError("GraphDecoder: spec_stats() needs a decoder built with speculative=k")
        steps, tokens = self.s_stats.tolist()
        return steps, tokens

    @torch.no_grad()
    def generate(self, prompt, new_tokens, return_prefill_logits=False, do_sample=False, temperature=1.0, top_k=0, top_p=1.0,
                 seed=0, eos_token_id=None, pad_token_id=None, append=False, prefill_chunk=None, attention_mask=None, speculate=None):
        """prompt [batch, P] int64 on the model's device -> [batch, P + new_tokens].  ``append=True`` continues the conversation
        the cache holds (a second turn): the token the previous ``generate`` emitted last, which the cache has not seen yet, and
        the prompt are written behind the cached rows, so the cache holds every token the caller has seen, in order; positions
        continue, the graphs are replayed as they were captured, and the return value is this turn's prompt and new tokens.  On
        an empty decoder it is a plain ``generate``.  ``prefill_chunk``: see ``prefill``.  On a decoder built with ``sampling=True``:
        ``do_sample`` draws every token by temperature / top-k / top-p sampling (``seed``: the 64-bit Philox key; token i of
        row b uses counter (i, b), so one seed gives one output), otherwise the argmax; a row that emits ``eos_token_id`` is
        finished (``self.done``) and holds ``pad_token_id`` (default 0) from the next position on.
        ``attention_mask`` (a decoder built with ``ragged=True`` only): the keep flags of a left-padded prompt, see ``prefill``; the
        return value holds the pad columns as given.
        ``speculate``: ``None`` = on exactly when the decoder was built with ``speculative=k``; ``True`` on a plain decoder raises;
        ``False`` on a speculative one runs the plain graphs (and keeps ``s_hist`` up to date).  A speculative call needs
        ``k`` cache rows beyond the last token's -- a verify pass writes up to k rows past the last kept one -- replays the verify
        graph in batches of ceil(left / (k + 1)) with ONE host read of the output column after each batch, and stops exactly at
        ``new_tokens`` (``s_limit`` clamps the last step on the device).  ``rows``, ``s_tok`` and the cache mean what they mean
        after a plain call, so ``append=True`` turns mix freely.  ``spec_stats()`` reports the steps it took."""
        B, P = prompt.shape
        if speculate is None:
            speculate = bool(self.speculative)
        elif speculate and not self.speculative:
            raise ValueError("GraphDecoder: speculate=True needs a decoder built with speculative=k")
        speculate = bool(speculate)
        if attention_mask is not None and append:
            raise ValueError("GraphDecoder: append=True takes no attention_mask: a second turn that is itself ragged would put pads "
                             "in the middle of the cache")
        if self.kv_bits == 8 and not self.kv8_append and (append or prefill_chunk is not None):
            raise ValueError("GraphDecoder: an int8 cache (kv_bits=8) takes fresh whole prompts only unless the decoder was "
                             "built with kv8_append=True: append=True and prefill_chunk then attend quantised rows")
        append = bool(append) and (self.rows > 0 or self._pending)
        feed = torch.cat([self.s_tok, prompt], dim=1) if append and self._pending else prompt
        start = self.rows if append else 0
        fed = start + feed.shape[1]                      # cache rows once the prompt is in
        if B != self.batch or fed + new_tokens > self.max_len:
            raise ValueError("GraphDecoder: built for batch %d and %d cache rows" % (self.batch, self.max_len))
        if speculate and fed + new_tokens + self.speculative > self.max_len:
            raise ValueError("GraphDecoder: a speculative generate needs %d spare cache rows (a verify pass writes up to k rows past "
                             "the last kept one): %d rows fed + %d new tokens + %d > %d cache rows"
                             % (self.speculative, fed, new_tokens, self.speculative, self.max_len))
        if not self.sampling:
            if (do_sample or temperature != 1.0 or top_k != 0 or top_p != 1.0 or seed != 0 or eos_token_id is not None
                    or pad_token_id is not None):
                raise ValueError("GraphDecoder: sampling and EOS arguments need a decoder built with sampling=True")
            out = self.prefill(feed, chunk=prefill_chunk, append=append, attention_mask=attention_mask)
            tok = out.logits[:, -1].argmax(-1, keepdim=True)
            self.out_buf[:, :1].copy_(tok)
            self.s_tok.copy_(tok)
            self.s_pos.fill_(fed)
            self.s_idx.fill_(1)
        else:
            from .. import ops
            from ..sampling import sampling_params
            sampling_params(temperature=float(temperature) if do_sample else 0.0, top_k=top_k, top_p=top_p, seed=seed,
                            eos_token_id=eos_token_id, pad_token_id=0 if pad_token_id is None else pad_token_id, out=self.params)
            self.done.zero_()
            out = self.prefill(feed, chunk=prefill_chunk, append=append, attention_mask=attention_mask)
            # the first token: the same op on the prompt's logits at column 0 (it leaves position = rows fed, column = 1)
            self.s_pos.fill_(fed - 1)
            self.s_idx.fill_(0)
            last = out.logits[:, -1]
            ops.sample_handover(last if last.stride(-1) == 1 else last.contiguous(), self.out_buf, self.s_idx, self.s_tok, self.s_pos, self.params,
                                self.done)
        left = new_tokens - 1
        if self.speculative:
            self.s_stats.zero_()
            if new_tokens >= 1:
                self.s_hist[:, fed:fed + 1].copy_(self.s_tok)   # the pending token's column is its cache row to be
        if speculate and left > 0:
            k = self.speculative
            self.s_limit.fill_(new_tokens)
            while left > 0:
                for _ in range(-(-left // (k + 1))):   # the fewest steps that can finish; the device clamp forbids an overshoot
                    if self.graph_spec is not None:
                        self.graph_spec.replay()
                    else:
                        self._advance_spec()
                left = new_tokens - int(self.s_idx)    # the one host read of a batch
        while left > 0:
            if self.graph_n is not None and left >= self.steps_per_graph:
                self.graph_n.replay()
                left -= self.steps_per_graph
            elif self.graph is not None:
                self.graph.replay()
                left -= 1
            else:
                with self._promise():
                    self._advance()
                left -= 1
        if self.speculative and not speculate and new_tokens > 1:   # the plain graphs do not keep the history
            self.s_hist[:, fed + 1:fed + new_tokens].copy_(self.out_buf[:, 1:new_tokens])
        if new_tokens >= 1:   # every emitted token but the last has been fed back and cached
            self.rows, self._pending = fed + new_tokens - 1, True
        tokens = torch.cat([prompt, self.out_buf[:, :new_tokens]], dim=1)
        return (tokens, out.logits[:, -1]) if return_prefill_logits else tokens

    def prefill(self, prompt, chunk=None, append=False, attention_mask=None):
        """Run the (unpadded) prompt [batch, P] eagerly; returns the model output of the last piece, whose logits hold the LAST
        position only where the model's forward can be told so.  By default the cache is emptied first.  ``chunk=c``: the
        prompt runs in pieces of at most ``c`` tokens, each behind the rows already written (activations are [batch, c, .]
        instead of [batch, P, .]).  ``append=True``: the prompt starts behind the rows the cache holds (``self.rows``) instead
        of emptying it.  Accelerated models attend the first piece of an emptied cache under ``fresh_static_prefill`` and every
        other piece under ``appended_static_prefill`` (``int8_rows=True`` on a decoder built with ``kv8_append=True``); other
        models run the same calls on their stock path.
        ``attention_mask`` (a decoder built with ``ragged=True`` only; ``None`` there means all ones): [batch, P] keep flags of a
        LEFT-padded batch (``left_pad_starts`` checks it: one host read).  Row b's first real column becomes ``s_start[b]``, the
        pieces run with ``position_ids`` counted from it (pads: 0), and the attention blocks neither attend nor read the pad rows
        (``llama_modules.padded_static_batch``); what the pad tokens left in the cache is never read.  The last column is real in
        every row.  With ``append=True`` a mask raises; without one the first turn's starts persist."""
        P = prompt.shape[1]
        if attention_mask is not None:
            if not self.ragged:
                raise ValueError("GraphDecoder: attention_mask needs a decoder built with ragged=True")
            if append:
                raise ValueError("GraphDecoder: append=True takes no attention_mask: a second turn that is itself ragged would put "
                                 "pads in the middle of the cache")
            if tuple(attention_mask.shape) != tuple(prompt.shape):
                raise ValueError("GraphDecoder: attention_mask must have the prompt's shape [batch, P]")
            starts = left_pad_starts(attention_mask)
        if self.kv_bits == 8 and not self.kv8_append and (append or chunk is not None):
            raise ValueError("GraphDecoder: an int8 cache (kv_bits=8) takes fresh whole prompts only unless the decoder was "
                             "built with kv8_append=True: append=True and chunk= then attend quantised rows")
        start = self.rows if append else 0
        if start + P > self.max_len:
            raise ValueError("GraphDecoder: built for batch %d and %d cache rows" % (self.batch, self.max_len))
        if chunk is not None and int(chunk) < 1:
            raise ValueError("GraphDecoder: chunk must be at least 1")
        step = P if chunk is None else int(chunk)
        if self.rolling:   # a ring admits pieces of at most rolling_chunk rows
            step = min(step, self.rolling_chunk)
        fresh = self._fresh_prefill_ok()
        from ..modules.llama_modules import appended_static_prefill, fresh_static_prefill
        if not append:
            if fresh:
                # every layer is an accelerated block on an initialised static cache: only the token counters are reset (the model
                # derives the prompt's positions from them; the blocks never read a row at or beyond the counter, so the stock
                # reset's zero-fill of 2 x layers cache tensors buys nothing), and the prompt is attended causally over its own
                # rows (llama_modules.fresh_static_prefill)
                torch._foreach_zero_([layer.cumulative_length for layer in self.cache.layers])   # one launch for all layers
            else:
                self.cache.reset()
        if self.ragged and not append:
            if attention_mask is None:
                self.s_start.zero_()
            else:
                self.s_start.copy_(starts)
        out = None
        for c0 in range(0, P, step):
            c1 = min(P, c0 + step)
            rows = torch.arange(start + c0, start + c1, device=prompt.device)
            # ragged: a token's position counts from its row's first real token (pads: 0)
            ragged_pos = {"position_ids": (rows[None, :] - self.s_start[:, None]).clamp_min(0)} if self.ragged else {}
            if not fresh:
                ctx = contextlib.nullcontext()
            elif c0 == 0 and not append:
                ctx = fresh_static_prefill()
            else:   # behind rows 0 .. start + c0 - 1, which are this sequence's tokens (llama_modules.appended_static_prefill)
                ctx = appended_static_prefill(int8_rows=True) if self.kv8_append else appended_static_prefill()
            with ctx, self._promise():
                out = self.model(prompt[:, c0:c1], past_key_values=self.cache, cache_position=rows, use_cache=True,
                                 **ragged_pos, **self._last_logits_only)
        if self.speculative:   # a token's column in the history is its cache row
            self.s_hist[:, start:start + P].copy_(prompt)
        self.rows, self._pending = start + P, False
        return out
