"""Quantised linear modules over the W8A16 operators.

Host-side mirror of /root/reference/python/eetq/modules/qlinear.py: ``quantize_and_preprocess_weights``
(:14-24), ``W8A16Linear`` (:27-62), ``EetqLinearMMFunction`` (:64-94) and ``EetqLinear`` (:96-124) keep
their names, constructor arguments, buffer names/shapes/dtypes and forward semantics.  ``W8A16LoraLinear``
(:127-186) is dead code in the reference (never constructed successfully) and is not carried over.

Layouts.  In memory the int8 buffer (``qweight`` / ``weight``) holds this library's ``gfx950`` layout -- NOT the bytes a
CUDA build of the reference keeps there.  State dicts are interchangeable all the same: every module re-encodes its int8
buffer to the reference's processed layout (``sm80``) when ``state_dict()`` is taken and back when ``load_state_dict()``
runs (eetq_amd/checkpoint.py), so a checkpoint written here loads in CUDA-EETQ and an NVIDIA-written one loads
here.  Code that copies tensors straight into the buffers (bypassing ``load_state_dict``) must convert them itself:
``eetq_amd.utils.convert_model_layout_(model, "sm80")``.
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from ..ops import (moe_router, moe_router_sigmoid, preprocess_weights, quant_weights, w4_a16_moe, w4_a16_moe_block,
                   w4_a16_gemm_t, w4_a16_gemm_tiled, w4_a16_gemm_tiled_supported, w4_a16_moe_direct_supported,
                   w4_a16_moe_backward, w4_a16_moe_block_sigmoid, w4_a16_moe_train, w8_a16_gemm, w8_a16_gemm_t, w8_a16_moe, w8_a16_moe_backward, w8_a16_moe_block,
                   w8_a16_moe_block_sigmoid, w8_a16_moe_train)
from ..checkpoint import install_layout_hooks

__all__ = ["quantize_and_preprocess_weights", "W8A16Linear", "W4A16Linear", "W8A16Experts", "W4A16Experts", "EetqLinearMMFunction", "EetqLinear", "input_grad",
           "W4A16LinearMMFunction", "input_grad_i4",
           "W8A16MoeFunction", "W4A16MoeFunction", "EetqTopKRouter", "EetqSparseMoeBlock"]


def quantize_and_preprocess_weights(weight, scales=None):
    """nn.Linear weight [out, in] -> (processed int8 [in, out], scales [out]).

    fp16 weights are quantised (per output channel, symmetric); int8 weights (e.g. bitsandbytes) are only
    re-laid-out and need caller-provided ``scales``.  Anything else raises ValueError, like the reference.
    Unlike the reference (which always round-trips through host memory, qlinear.py:16), a weight that
    already lives on the GPU is quantised in place on that GPU.
    """
    kn = torch.t(weight).contiguous()  # [K = in_features, N = out_features]
    if weight.dtype == torch.int8:
        assert scales is not None, "int8 weights need their scales"
        return preprocess_weights(kn), scales
    if weight.dtype == torch.float16:
        processed, scales = quant_weights(kn, torch.int8, False)
        return processed, scales
    raise ValueError("Unsupported data type: {}".format(weight.dtype))


class W8A16Linear(nn.Module):
    """Linear layer over an int8 weight ``qweight`` [in, out], fp16 ``weight_scales`` [out].  Inference-only unless ``trainable``
    is set (``eet_quantize(..., trainable=True)`` or ``utils.set_trainable``): then a call in grad mode whose input requires grad
    and that passes no extension argument runs through :class:`EetqLinearMMFunction` -- the same output bits, and an input
    gradient from ``w8_a16_gemm_t`` (the int8 weight stays frozen)."""

    trainable = False   # a plain attribute, not a buffer: state dicts do not change

    def __init__(self, in_features, out_features, bias=True, dev="cuda:0"):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.register_buffer("qweight", torch.zeros((in_features, out_features), dtype=torch.int8, device=dev))
        self.register_buffer("weight_scales", torch.zeros((out_features,), dtype=torch.float16, device=dev))
        if bias:
            self.register_buffer("bias", torch.zeros((out_features,), dtype=torch.float16, device=dev))
        else:
            self.bias = None
        # state dicts carry the reference's layout: re-encode on save / load (see the module docstring)
        self.checkpoint_layout = None   # None = the process-wide wire layout; "sm80" / "gfx950" pins what load expects
        install_layout_hooks(self, "qweight")

    @classmethod
    def from_torch(cls, linear, scales=None, init_only=False):
        dev = linear.weight.device
        mod = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, dev=dev)
        if init_only:  # buffers only; weights arrive later through load_state_dict
            return mod
        if linear.bias is not None:
            mod.bias = linear.bias.clone().half()
        qweight, scales = quantize_and_preprocess_weights(linear.weight, scales)
        mod.qweight = qweight.to(dev)
        mod.weight_scales = scales.half().to(dev)
        return mod

    def forward(self, input, residual=None, norm=None, gated=False, activation=""):
        if (self.trainable and torch.is_grad_enabled() and input.requires_grad and residual is None and norm is None
                and not gated and not activation):
            return EetqLinearMMFunction.apply(input, self.qweight, self.weight_scales, self.bias)
        with torch.no_grad():
            return self._forward(input, residual, norm, gated, activation)

    def _forward(self, input, residual, norm, gated, activation):
        # bias is fused into the kernel epilogue: same bits as the reference's `output + self.bias` (qlinear.py:61);
        # `residual` (extension) is added after it in the same epilogue: the decoder block's `residual + proj(x)`
        # `norm=(gamma, eps)` (extension): RMS-norm of the input, fused into the launch for single-row inputs
        # `gated=True` (extension): input is a fused gate|up block and the projection runs on silu(gate) * up
        # `activation` (extension): "relu" / "gelu" / "silu" epilogues, "silu_glu8" for a gate|up weight in glu8 column order
        return w8_a16_gemm(input, self.qweight, self.weight_scales, bias=self.bias, residual=residual, norm=norm,
                           gated=gated, activation=activation)

    def extra_repr(self):
        return "in_features={}, out_features={}, bias={}".format(self.in_features, self.out_features,
                                                                 self.bias is not None)


class W4A16Linear(nn.Module):
    """int4 weight-only linear layer (extension; the reference binds int4 quantisation -- ``quant_weights(w, torch.quint4x2)``
    -- but no int4 GEMM): packed ``qweight`` int8 [in, out / 2] (two values per byte) in the gfx950 int4 layout, fp16
    ``weight_scales`` [out].  Needs in_features % 128 == 0 and out_features % 16 == 0.  Inference-only unless ``trainable`` is
    set (``eet_quantize(..., bits=4, trainable=True)`` or ``utils.set_trainable``): then a call in grad mode whose input requires
    grad and that passes no ``residual`` runs through :class:`W4A16LinearMMFunction` -- the same output bits, and an input
    gradient from ``w4_a16_gemm_t`` (the int4 weight stays frozen).

    ``prompt_path`` (a plain attribute, not a buffer: state dicts do not change; ``utils.set_prompt_path`` sets it on a model) chooses
    what serves calls with more than 128 rows: ``"auto"``, the default, is ``w8_a16_gemm``'s rule (the nibbles are expanded to int8
    tiles in a per-stream scratch buffer, then the W8A16 kernels run); ``"direct"`` sends such a call, where
    ``ops.w4_a16_gemm_tiled_supported`` takes its shape, to the tiled kernel on the int4 tiles themselves (``ops.w4_a16_gemm_tiled``,
    DESIGN.md 4.8) -- no expansion, no scratch, capturable cold -- and leaves every other call as it is."""

    trainable = False   # a plain attribute, not a buffer: state dicts do not change

    prompt_path = "auto"
    PROMPT_PATHS = ("auto", "direct")
    DIRECT_MIN_ROWS = 129   # up to 128 rows AUTO already reads the int4 tiles (GEMV, stream kernel, split-K tile)

    def __init__(self, in_features, out_features, bias=True, dev="cuda:0"):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.register_buffer("qweight", torch.zeros((in_features, out_features // 2), dtype=torch.int8, device=dev))
        self.register_buffer("weight_scales", torch.zeros((out_features,), dtype=torch.float16, device=dev))
        if bias:
            self.register_buffer("bias", torch.zeros((out_features,), dtype=torch.float16, device=dev))
        else:
            self.bias = None

    @classmethod
    def from_torch(cls, linear, init_only=False):
        dev = linear.weight.device
        mod = cls(linear.in_features, linear.out_features, bias=linear.bias is not None, dev=dev)
        if init_only:
            return mod
        if linear.weight.dtype != torch.float16:
            raise ValueError("Unsupported data type: {}".format(linear.weight.dtype))
        if linear.bias is not None:
            mod.bias = linear.bias.clone().half()
        qweight, scales = quant_weights(torch.t(linear.weight).contiguous(), torch.quint4x2, False)
        mod.qweight = qweight.to(dev)
        mod.weight_scales = scales.half().to(dev)
        return mod

    def route(self, rows):
        """``"direct"`` when a call with ``rows`` flattened input rows runs ``ops.w4_a16_gemm_tiled``, else ``"auto"`` (shapes and
        ``prompt_path`` only; no GPU work)."""
        if self.prompt_path == "auto":
            return "auto"
        if self.prompt_path != "direct":
            raise ValueError("W4A16Linear.prompt_path must be one of %r (got %r)" % (self.PROMPT_PATHS, self.prompt_path))
        direct = rows >= self.DIRECT_MIN_ROWS and w4_a16_gemm_tiled_supported(rows, self.out_features, self.in_features)
        return "direct" if direct else "auto"

    def forward(self, input, residual=None):
        direct = self.route(input.numel() // self.in_features if self.in_features else 0) == "direct"
        if self.trainable and torch.is_grad_enabled() and input.requires_grad and residual is None:
            return W4A16LinearMMFunction.apply(input, self.qweight, self.weight_scales, self.bias, direct)
        with torch.no_grad():
            if direct:
                return w4_a16_gemm_tiled(input, self.qweight, self.weight_scales, bias=self.bias, residual=residual)
            return w8_a16_gemm(input, self.qweight, self.weight_scales, bias=self.bias, residual=residual)

    def extra_repr(self):
        return "in_features={}, out_features={}, bias={}, bits=4".format(self.in_features, self.out_features,
                                                                        self.bias is not None)


class _QuantExperts(nn.Module):
    """What :class:`W8A16Experts` and :class:`W4A16Experts` share: the four buffers (``bits`` per weight, 8 / bits values per byte
    along the last dimension), the scaffolding of :meth:`from_experts` and ``extra_repr``.  A subclass sets ``bits`` and gives
    ``unsupported_reason``, ``_quantize_gate_up`` and ``forward``."""

    bits = None

    def __init__(self, num_experts, hidden_dim, intermediate_dim, dev="cuda:0"):
        super().__init__()
        self.num_experts = num_experts
        self.hidden_dim = hidden_dim
        self.intermediate_dim = intermediate_dim
        E, H, I, pack = num_experts, hidden_dim, intermediate_dim, 8 // self.bits
        self.register_buffer("gate_up_qweight", torch.zeros((E, H, 2 * I // pack), dtype=torch.int8, device=dev))
        self.register_buffer("gate_up_scales", torch.zeros((E, 2 * I), dtype=torch.float16, device=dev))
        self.register_buffer("down_qweight", torch.zeros((E, I, H // pack), dtype=torch.int8, device=dev))
        self.register_buffer("down_scales", torch.zeros((E, H), dtype=torch.float16, device=dev))

    @classmethod
    def from_experts(cls, module, init_only=False):
        """Quantise a transformers experts module (see :meth:`unsupported_reason` for what is taken; anything else raises
        ValueError before any GPU work).  Each expert is quantised per output channel by ``ops.quant_weights``."""
        why = cls.unsupported_reason(module)
        if why is not None:
            raise ValueError("%s.from_experts: %s: %s" % (cls.__name__, type(module).__name__, why))
        gu, dn = module.gate_up_proj, module.down_proj
        E, n2, H = gu.shape
        mod = cls(E, H, n2 // 2, dev=gu.device)
        if init_only:
            return mod
        if gu.dtype != torch.float16 or dn.dtype != torch.float16:
            raise ValueError("Unsupported data type: {}".format(gu.dtype))
        with torch.no_grad():
            q, s = cls._quantize_gate_up(gu.detach().transpose(1, 2))  # from [E, H, 2I] gate | up
            mod.gate_up_qweight = q.to(gu.device)
            mod.gate_up_scales = s.to(gu.device)
            q, s = quant_weights(dn.detach().transpose(1, 2).contiguous(), torch.int8 if cls.bits == 8 else torch.quint4x2, False)
            mod.down_qweight = q.to(gu.device)  # [E, I, H * bits / 8]
            mod.down_scales = s.half().to(gu.device)
        return mod

    def extra_repr(self):
        return "num_experts={}, hidden_dim={}, intermediate_dim={}{}".format(self.num_experts, self.hidden_dim, self.intermediate_dim,
                                                                             "" if self.bits == 8 else ", bits=%d" % self.bits)


class W8A16Experts(_QuantExperts):
    """int8 stand-in for transformers' 3-D experts modules (``MixtralExperts``, ``Qwen3MoeExperts``, ...): same forward signature
    ``(hidden_states [T, H], top_k_index [T, k], top_k_weights [T, k]) -> [T, H]``, so the MoE block's ``self.experts(...)`` call
    is unchanged.  Buffers: ``gate_up_qweight`` int8 [E, H, 2I] (per expert the gfx950 layout, columns in glu8 order: 8 gate + the
    matching 8 up per 16-column tile), ``gate_up_scales`` fp16 [E, 2I] (same order), ``down_qweight`` int8 [E, I, H],
    ``down_scales`` fp16 [E, H].  Runs ``ops.w8_a16_moe``.

    Inference-only unless ``trainable`` is set (``eet_quantize(..., trainable=True)`` or ``utils.set_trainable``): then a call in
    grad mode with ``hidden_states`` or ``top_k_weights`` requiring grad runs through :class:`W8A16MoeFunction` -- the same
    output bits, and gradients for both (the int8 stacks stay frozen).

    State dicts hold the stacks in this library's gfx950 layout, unlike W8A16Linear's: the reference has no experts module, so
    there is no CUDA-written checkpoint to stay compatible with, and the glu8 column order has no counterpart in its layout."""

    trainable = False   # a plain attribute, not a buffer: state dicts do not change

    bits = 8

    @staticmethod
    def unsupported_reason(module):
        """None when :meth:`from_experts` takes ``module``, else why not."""
        gu, dn = getattr(module, "gate_up_proj", None), getattr(module, "down_proj", None)
        if not isinstance(gu, torch.Tensor) or not isinstance(dn, torch.Tensor) or gu.dim() != 3 or dn.dim() != 3:
            return "no 3-D gate_up_proj / down_proj"
        if not getattr(module, "has_gate", False) or not getattr(module, "is_concatenated", False):
            return "needs a concatenated [gate; up] projection (has_gate, is_concatenated)"
        if getattr(module, "is_transposed", False):
            return "transposed expert weights are not supported"
        if getattr(module, "has_bias", False):
            return "expert biases are not supported"
        act = getattr(module, "act_fn", None)
        if not isinstance(act, nn.SiLU) and type(act).__name__ != "SiLUActivation":
            return "the activation must be SiLU (got %s)" % type(act).__name__
        E, n2, H = gu.shape
        if n2 % 2 or dn.shape != (E, H, n2 // 2):
            return "gate_up_proj [E, 2I, H] and down_proj [E, H, I] do not match"
        if H % 64 or (n2 // 2) % 64:
            return "the gfx950 layout needs H %% 64 == 0 and I %% 64 == 0 (H = %d, I = %d)" % (H, n2 // 2)
        return None

    @staticmethod
    def _quantize_gate_up(w):
        """int8 tiles and scales of the [E, H, 2I] gate | up weights: quantised in that order, then put in glu8 order"""
        from ..utils.fuse import _glu8_interleave_columns, _glu8_interleave_tiles
        E, H, n2 = w.shape
        q, s = quant_weights(w.contiguous(), torch.int8, False)
        halves = q.reshape(E, 2, -1)  # per expert: the I/16 gate tile rows, then the I/16 up tile rows
        return (_glu8_interleave_tiles(halves[:, 0], halves[:, 1], H).reshape(E, H, n2),
                _glu8_interleave_columns(s[:, :n2 // 2], s[:, n2 // 2:]).half().contiguous())

    def forward(self, hidden_states, top_k_index, top_k_weights):
        """Any number of tokens: four launches (five when trainable), no host sync, capturable in a graph.  The two grouped GEMMs run
        the decode kernel at T <= 16 or fewer than 16 rows per expert on average, the grouped tiled kernel above -- chosen from the
        shapes, never from the routing."""
        if (self.trainable and torch.is_grad_enabled()
                and (hidden_states.requires_grad or top_k_weights.requires_grad)):
            return W8A16MoeFunction.apply(hidden_states, top_k_index, top_k_weights, self.gate_up_qweight, self.gate_up_scales,
                                          self.down_qweight, self.down_scales)
        with torch.no_grad():
            return w8_a16_moe(hidden_states, top_k_index, top_k_weights, self.gate_up_qweight, self.gate_up_scales,
                              self.down_qweight, self.down_scales)


class W4A16Experts(_QuantExperts):
    """int4 stand-in for transformers' 3-D experts modules: :class:`W8A16Experts` at half the expert bytes, same
    forward signature.  Buffers: ``gate_up_qweight`` int8 [E, H, I] (= [E, K = H, N / 2] with N = 2I: two values per byte; per expert
    the gfx950 int4 layout of its [H, 2I] weight, columns in glu8 order: 8 gate + the matching 8 up per 16-column tile),
    ``gate_up_scales`` fp16 [E, 2I] (same order), ``down_qweight`` int8 [E, I, H / 2], ``down_scales`` fp16 [E, H].  Needs
    H % 128 == 0 and I % 128 == 0 (int4 tiles are 128 deep).  Runs ``ops.w4_a16_moe``.

    ``prompt_path`` (a plain attribute, not a buffer: state dicts do not change; ``eet_quantize(..., expert_prompt_path=...)`` sets
    it) chooses what serves prompts: ``"auto"``, the default, is the op's own rule (the decode kernel, or from 64 rows per expert
    the expansion to int8 tiles); ``"direct"`` sends a call with T > 16, T k >= 16 E (the int8 layer's seam) and both projections
    inside ``ops.w4_a16_moe_direct_supported`` to the grouped tiled kernel on the int4 tiles themselves -- the bits of the expanded
    path, no [E, K, N] buffer -- and every other call to the decode kernel; the expansion is never used in this mode.

    Inference-only unless ``trainable`` is set (``utils.set_trainable(model, True, int4_experts=True)``; the two-argument call
    passes int4 experts by): then a call in grad mode with ``hidden_states`` or ``top_k_weights`` requiring grad runs through
    :class:`W4A16MoeFunction` -- the same output bits on the same path, and gradients for both (the int4 stacks stay frozen and
    are read as int4 tiles, never expanded, by the backward).  Every other call returns a detached output.
    State dicts hold the four buffers as they are, like :class:`W8A16Experts`."""

    trainable = False   # a plain attribute, not a buffer: state dicts do not change

    bits = 4

    prompt_path = "auto"
    PROMPT_PATHS = ("auto", "direct")

    def op_path(self, T, k):
        """The ``path`` argument of the int4 ops for a call with T tokens and k choices per token (shapes only, never the routing)."""
        if self.prompt_path == "auto":
            return "auto"
        if self.prompt_path != "direct":
            raise ValueError("W4A16Experts.prompt_path must be one of %r (got %r)" % (self.PROMPT_PATHS, self.prompt_path))
        E, H, I = self.num_experts, self.hidden_dim, self.intermediate_dim
        direct = T > 16 and T * k >= 16 * E and w4_a16_moe_direct_supported(T, k, E, H, I)
        return "direct" if direct else "decode"

    @staticmethod
    def unsupported_reason(module):
        """None when :meth:`from_experts` takes ``module``, else why not: :meth:`W8A16Experts.unsupported_reason`'s rules, and
        H and I multiples of 128."""
        why = W8A16Experts.unsupported_reason(module)
        if why is not None:
            return why
        _, n2, H = module.gate_up_proj.shape
        if H % 128 or (n2 // 2) % 128:
            return "the gfx950 int4 layout needs H %% 128 == 0 and I %% 128 == 0 (H = %d, I = %d)" % (H, n2 // 2)
        return None

    @staticmethod
    def _quantize_gate_up(w):
        """Per-channel quantisation commutes with a permutation of the output channels, so the gate|up columns are put in glu8
        order in fp16 and each expert is then quantised and packed by ``ops.quant_weights(w, torch.quint4x2)``."""
        from ..utils.fuse import _glu8_interleave_columns
        I = w.shape[2] // 2
        q, s = quant_weights(_glu8_interleave_columns(w[..., :I], w[..., I:]).contiguous(), torch.quint4x2, False)
        return q, s.half()

    def forward(self, hidden_states, top_k_index, top_k_weights):
        """Any number of tokens, no host sync, capturable in a graph.  Four launches on the int4 decode kernel (five when
        trainable); on the prompt path (``ops.w4_a16_moe_path``: chosen from the shapes, never from the routing) each projection's
        stack is first expanded to int8 tiles and runs the grouped tiled W8A16 kernel.  With ``prompt_path = "direct"`` prompts
        run the grouped tiled kernel on the int4 tiles instead (see the class)."""
        path = self.op_path(hidden_states.shape[0], top_k_index.shape[1])
        if (self.trainable and torch.is_grad_enabled()
                and (hidden_states.requires_grad or top_k_weights.requires_grad)):
            return W4A16MoeFunction.apply(hidden_states, top_k_index, top_k_weights, self.gate_up_qweight, self.gate_up_scales,
                                          self.down_qweight, self.down_scales, path)
        with torch.no_grad():
            return w4_a16_moe(hidden_states, top_k_index, top_k_weights, self.gate_up_qweight, self.gate_up_scales,
                              self.down_qweight, self.down_scales, path)


def _adopt(module, mixin):
    """Give ``module`` the class ``mixin`` in place: a subclass of (mixin, type(module)) named after the mixin, made once per
    original class.  The module keeps its parameters, buffers, attributes and hooks, stays an instance of its original class (what
    transformers' output recorders match on) and finds the original forward as ``_eetq_base.forward``.  The subclass exists only
    in the process that made it: ``state_dict()`` / ``load_state_dict()`` are unaffected, but pickling a whole converted model
    (``torch.save(model)``) is not supported -- save the state dict and run ``eet_quantize(..., router=True)`` on the loading side."""
    base = type(module)
    if isinstance(module, mixin):
        return module
    sub = mixin._adopted.get(base)
    if sub is None:
        sub = type(mixin.__name__, (mixin, base), {"__module__": mixin.__module__, "_eetq_base": base})
        mixin._adopted[base] = sub
    module.__class__ = sub
    return module


def _observed(module):
    """True when forward hooks (the module's own or global ones) would see a call of ``module``"""
    from torch.nn.modules import module as _m
    return bool(module._forward_hooks or module._forward_pre_hooks or _m._global_forward_hooks or _m._global_forward_pre_hooks)


class EetqTopKRouter(nn.Module):
    """Drop-in for transformers' softmax top-k routers -- ``MixtralTopKRouter``, ``Qwen2MoeTopKRouter``, ``Qwen3MoeTopKRouter``,
    ``OlmoeTopKRouter`` (by class name) -- on ``ops.moe_router``: one launch at T <= 16 instead of
    ``F.linear -> softmax -> topk -> sum -> div (-> .to)``.  Same parameter (``weight`` [E, H]: state-dict keys do not change), same
    return triple ``(router_logits [T, E], router_scores [T, k], router_indices int64 [T, k])`` and score dtype: Mixtral float32 and
    always renormalised, the others ``norm_topk_prob`` and the logits' dtype.

    :meth:`from_router` converts a router in place and keeps it an instance of its original class.  When grad mode is on and
    ``hidden_states`` or ``weight`` requires grad, the call runs the original torch forward, so router training and the auxiliary
    loss keep their autograd path; everything else needs fp16 GPU tensors, E <= 256, top_k <= 16 and H % 64 == 0.

    The sigmoid, bias-corrected, group-limited routers whose forward is DeepSeek-V3's program text -- ``SIGMOID_CLASS_NAMES`` -- are
    adopted the same way, on ``ops.moe_router_sigmoid``: the return triple is theirs, ``(router_logits fp32 [T, E],
    topk_weights fp32 [T, k], topk_indices int64 [T, k])``, and the ``e_score_correction_bias`` buffer stays where it is."""

    SIGMOID_CLASS_NAMES = ("DeepseekV3TopkRouter", "DeepseekV32TopkRouter", "Glm4MoeTopkRouter", "Glm4MoeLiteTopkRouter",
                           "Dots1TopkRouter", "SolarOpenTopkRouter")
    CLASS_NAMES = ("MixtralTopKRouter", "Qwen2MoeTopKRouter", "Qwen3MoeTopKRouter", "OlmoeTopKRouter") + SIGMOID_CLASS_NAMES
    _adopted = {}
    _eetq_base = None

    def __init__(self, num_experts, hidden_dim, top_k, norm_topk_prob=True, scores_dtype=None, dev=None):
        """A stand-alone router (``scores_dtype`` None: the logits' dtype, like the Qwen / OLMoE routers)"""
        super().__init__()
        self.num_experts, self.hidden_dim, self.top_k = num_experts, hidden_dim, top_k
        self.norm_topk_prob = norm_topk_prob
        self._scores_dtype = scores_dtype
        self.weight = nn.Parameter(torch.zeros(num_experts, hidden_dim, dtype=torch.float16, device=dev))

    @classmethod
    def unsupported_reason(cls, module):
        """None when :meth:`from_router` takes ``module``, else why not."""
        if isinstance(module, cls):
            return None
        if type(module).__name__ not in cls.CLASS_NAMES:
            return "%s is not one of %s" % (type(module).__name__, ", ".join(cls.CLASS_NAMES))
        w = getattr(module, "weight", None)
        if not isinstance(w, torch.Tensor) or w.dim() != 2:
            return "no 2-D weight"
        if w.dtype != torch.float16:
            return "the router kernel needs a float16 weight (got %s)" % str(w.dtype).replace("torch.", "")
        E, H = w.shape
        k = getattr(module, "top_k", None)
        if not isinstance(k, int) or not 1 <= k <= min(E, 16) or E > 256:
            return "the router kernel serves E <= 256 and top_k <= 16 (E = %d, top_k = %r)" % (E, k)
        if H % 64:
            return "the router kernel needs H %% 64 == 0 (H = %d)" % H
        if type(module).__name__ in cls.SIGMOID_CLASS_NAMES:
            return cls._sigmoid_unsupported_reason(module, E, k)
        return None

    @staticmethod
    def _sigmoid_unsupported_reason(module, E, k):
        """the sigmoid routers are matched by name, so everything their forward reads is required here"""
        missing = [a for a in ("num_group", "topk_group", "norm_topk_prob", "routed_scaling_factor", "e_score_correction_bias")
                   if getattr(module, a, None) is None]
        if missing:
            return "no %s" % ", ".join(missing)
        bias, G, KG = module.e_score_correction_bias, module.num_group, module.topk_group
        if not isinstance(bias, torch.Tensor) or bias.shape != (E,) or bias.dtype not in (torch.float16, torch.float32):
            return "e_score_correction_bias is not a float16 or float32 tensor [E]"
        if not isinstance(G, int) or not isinstance(KG, int) or not 1 <= G <= 64 or E % G or (G > 1 and E // G < 2):
            return ("the router kernel needs 1 <= n_group <= 64 dividing E into groups of at least two experts (E = %d, n_group = %r)"
                    % (E, G))
        if not 1 <= KG <= G or k > KG * (E // G):
            return "the router kernel needs 1 <= topk_group <= n_group and top_k <= topk_group * E / n_group (topk_group = %r)" % (KG,)
        scale = module.routed_scaling_factor
        if not isinstance(scale, (int, float)) or scale != scale or scale in (float("inf"), float("-inf")):
            return "routed_scaling_factor is not a finite number (%r)" % (scale,)
        return None

    @property
    def is_sigmoid(self):
        base = self._eetq_base
        return base is not None and base.__name__ in self.SIGMOID_CLASS_NAMES

    @classmethod
    def from_router(cls, module):
        why = cls.unsupported_reason(module)
        if why is not None:
            raise ValueError("EetqTopKRouter.from_router: %s" % why)
        return _adopt(module, cls)

    @property
    def renormalises(self):
        base = self._eetq_base
        return True if base is not None and base.__name__.startswith("Mixtral") else bool(self.norm_topk_prob)

    def scores_dtype(self, logits_dtype=torch.float16):
        base = self._eetq_base
        if base is not None:
            return torch.float32 if base.__name__.startswith("Mixtral") or self.is_sigmoid else logits_dtype
        return self._scores_dtype if self._scores_dtype is not None else logits_dtype

    def falls_back(self, hidden_states):
        """True when this call takes the torch forward: grad mode with a gradient to deliver"""
        return torch.is_grad_enabled() and (hidden_states.requires_grad or self.weight.requires_grad)

    def _torch_forward(self, hidden_states):
        if self._eetq_base is not None:
            return self._eetq_base.forward(self, hidden_states)
        logits = nn.functional.linear(hidden_states, self.weight)
        top, idx = torch.topk(nn.functional.softmax(logits, dtype=torch.float, dim=-1), self.top_k, dim=-1)
        if self.norm_topk_prob:
            top = top / top.sum(dim=-1, keepdim=True)
        return logits, top.to(self.scores_dtype(logits.dtype)), idx

    def forward(self, hidden_states):
        hidden_states = hidden_states.reshape(-1, self.hidden_dim)
        if self.falls_back(hidden_states):
            return self._torch_forward(hidden_states)
        with torch.no_grad():
            if self.is_sigmoid:
                return moe_router_sigmoid(hidden_states, self.weight, *self.sigmoid_args())
            return moe_router(hidden_states, self.weight, self.top_k, self.renormalises, self.scores_dtype())

    def sigmoid_args(self):
        """what ``ops.moe_router_sigmoid`` and the ``*_moe_block_sigmoid`` ops take after the router weight"""
        return (self.e_score_correction_bias, self.top_k, self.num_group, self.topk_group, bool(self.norm_topk_prob),
                float(self.routed_scaling_factor))

    def extra_repr(self):
        return "num_experts={}, hidden_dim={}, top_k={}".format(self.weight.shape[0], self.weight.shape[1], self.top_k)


class EetqSparseMoeBlock(nn.Module):
    """Drop-in for the sparse MoE blocks whose forward is exactly ``gate -> experts -> reshape`` -- ``MixtralSparseMoeBlock``,
    ``Qwen3MoeSparseMoeBlock``, ``OlmoeSparseMoeBlock`` (by class name) -- once their ``gate`` is an :class:`EetqTopKRouter` and their
    ``experts`` a :class:`W8A16Experts` / :class:`W4A16Experts`: the submodules keep their names, and in inference the block is
    ``ops.w8_a16_moe_block`` / ``ops.w4_a16_moe_block`` on their buffers (four launches at T <= 16), the bits of
    ``experts(hidden, *gate(hidden)[2:0:-1])``.

    The original forward (``gate`` then ``experts``, each through its ``__call__``) runs instead whenever the router would fall
    back (grad mode with a gradient to deliver), the experts are ``trainable`` in grad mode, a Mixtral block is in training mode
    with jitter noise > 0, or forward hooks observe ``gate`` or ``experts``.  The last rule is how ``output_router_logits=True``
    keeps working: transformers records the router's output with a forward hook on the gate.  It installs ALL of a model's
    recording hooks, the gates' included, the first time ANY ``output_*`` flag (``output_router_logits``, ``output_hidden_states``,
    ``output_attentions``) is asked for, and never removes them: from that call on every block of that model stays on the unfused
    path for the model's lifetime (the router swap still applies; :meth:`fused` tells).

    ``SHARED_CLASS_NAMES`` are the blocks around the sigmoid routers, whose forward is
    ``experts(x, *gate(x)[2:0:-1]) + shared_experts(x)``: fused, the routed half is ``ops.w8_a16_moe_block_sigmoid`` /
    ``ops.w4_a16_moe_block_sigmoid`` and the shared expert (quantised linears already) is added in the original's operand order, so
    the result is the bits of the unfused path.  Hooks observing ``shared_experts`` keep such a block unfused as well."""

    SHARED_CLASS_NAMES = ("DeepseekV3MoE", "DeepseekV32MoE", "Glm4MoeMoE", "Glm4MoeLiteMoE", "Dots1MoE", "SolarOpenMoE")
    CLASS_NAMES = ("MixtralSparseMoeBlock", "Qwen3MoeSparseMoeBlock", "OlmoeSparseMoeBlock") + SHARED_CLASS_NAMES
    _adopted = {}
    _eetq_base = None

    @classmethod
    def unsupported_reason(cls, module):
        """None when :meth:`from_block` takes ``module``, else why not."""
        if isinstance(module, cls):
            return None
        if type(module).__name__ not in cls.CLASS_NAMES:
            return "%s is not one of %s" % (type(module).__name__, ", ".join(cls.CLASS_NAMES))
        if not isinstance(getattr(module, "gate", None), EetqTopKRouter):
            return "its gate is not an EetqTopKRouter"
        if not isinstance(getattr(module, "experts", None), (W8A16Experts, W4A16Experts)):
            return "its experts are not quantised"
        shared = type(module).__name__ in cls.SHARED_CLASS_NAMES
        if shared != module.gate.is_sigmoid:
            return "its gate's routing rule is not the one its forward expects"
        if shared and not isinstance(getattr(module, "shared_experts", None), nn.Module):
            return "no shared_experts module"
        return None

    @classmethod
    def from_block(cls, module):
        why = cls.unsupported_reason(module)
        if why is not None:
            raise ValueError("EetqSparseMoeBlock.from_block: %s" % why)
        return _adopt(module, cls)

    def fused(self, hidden_states):
        """True when this call runs the block op"""
        gate, experts = self.gate, self.experts
        if gate.falls_back(hidden_states):
            return False
        if getattr(experts, "trainable", False) and torch.is_grad_enabled():
            return False
        if self.training and getattr(self, "jitter_noise", 0) > 0:
            return False
        if gate.is_sigmoid and _observed(self.shared_experts):
            return False
        return not (_observed(gate) or _observed(experts))

    def forward(self, hidden_states):
        if not self.fused(hidden_states):
            return self._eetq_base.forward(self, hidden_states)
        gate, experts = self.gate, self.experts
        flat = hidden_states.reshape(-1, hidden_states.shape[-1])
        if gate.is_sigmoid:
            args = (flat, gate.weight, *gate.sigmoid_args(), experts.gate_up_qweight, experts.gate_up_scales, experts.down_qweight,
                    experts.down_scales)
            with torch.no_grad():
                out = (w4_a16_moe_block_sigmoid(*args, experts.op_path(flat.shape[0], gate.top_k)) if experts.bits == 4
                       else w8_a16_moe_block_sigmoid(*args))
            return out.reshape(hidden_states.shape) + self.shared_experts(hidden_states)
        args = (flat, gate.weight, gate.top_k, gate.renormalises, gate.scores_dtype(), experts.gate_up_qweight, experts.gate_up_scales,
                experts.down_qweight, experts.down_scales)
        with torch.no_grad():
            out = w4_a16_moe_block(*args, experts.op_path(flat.shape[0], gate.top_k)) if experts.bits == 4 else w8_a16_moe_block(*args)
        return out.reshape(hidden_states.shape)


def input_grad(grad_output, weight, scales, x_shape, x_dtype=torch.float16):
    """``grad_output @ dequant(weight, scales).T`` shaped like the forward's input ``x_shape``: the input gradient of the W8A16
    projection.  An fp16 GPU gradient goes through ``w8_a16_gemm_t`` (the dequantised weight is never materialised); anything
    else through the reference's identity path (dequantise W by multiplying an identity -- exact: every output element is a
    single product -- then an fp16 GEMM in torch)."""
    if grad_output.dtype == torch.float16 and grad_output.is_cuda:
        return w8_a16_gemm_t(grad_output, weight, scales).reshape(x_shape)
    eye = torch.eye(weight.shape[0], device=weight.device, dtype=x_dtype)
    w_deq = w8_a16_gemm(eye, weight, scales)  # fp16 [K, N] == fp16(q * s)
    return grad_output.matmul(w_deq.transpose(0, 1)).reshape(x_shape)


class EetqLinearMMFunction(Function):
    """Autograd wrapper: forward = fused dequant GEMM; backward returns grad_input only (the int8 weight is frozen), computed
    by :func:`input_grad`.  ``x`` itself is not saved: no gradient here needs it."""

    @staticmethod
    def forward(ctx, x, weight, scales, bias=None):
        ctx.save_for_backward(weight, scales)
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        return w8_a16_gemm(x, weight, scales, bias=bias)

    @staticmethod
    def backward(ctx, grad_output):
        weight, scales = ctx.saved_tensors
        grad_input = None
        if ctx.needs_input_grad[0]:
            grad_input = input_grad(grad_output, weight, scales, ctx.x_shape, ctx.x_dtype)
        return grad_input, None, None, None


def input_grad_i4(grad_output, weight, scales, x_shape, x_dtype=torch.float16):
    """:func:`input_grad` for a packed int4 ``[K, N/2]`` weight: an fp16 GPU gradient goes through ``w4_a16_gemm_t`` (neither
    int8 tiles nor the dequantised weight are materialised); anything else through the identity path, which the forward operator
    accepts for int4 as it is."""
    if grad_output.dtype == torch.float16 and grad_output.is_cuda:
        return w4_a16_gemm_t(grad_output, weight, scales).reshape(x_shape)
    eye = torch.eye(weight.shape[0], device=weight.device, dtype=x_dtype)
    w_deq = w8_a16_gemm(eye, weight, scales)  # fp16 [K, N] == fp16(q * s)
    return grad_output.matmul(w_deq.transpose(0, 1)).reshape(x_shape)


class W4A16LinearMMFunction(Function):
    """:class:`EetqLinearMMFunction` over a packed int4 weight: forward = the fused int4 dequant GEMM (the bits of the module's
    inference call); backward returns grad_input only, computed by :func:`input_grad_i4`.  ``x`` is not saved.  ``direct``: the
    forward runs ``w4_a16_gemm_tiled`` (the module's ``prompt_path = "direct"`` route), as its inference call does."""

    @staticmethod
    def forward(ctx, x, weight, scales, bias=None, *direct):
        ctx.save_for_backward(weight, scales)
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        ctx.n_args = 4 + len(direct)   # the four-argument call of before keeps working
        if direct and direct[0]:
            return w4_a16_gemm_tiled(x, weight, scales, bias=bias)
        return w8_a16_gemm(x, weight, scales, bias=bias)

    @staticmethod
    def backward(ctx, grad_output):
        weight, scales = ctx.saved_tensors
        grad_input = None
        if ctx.needs_input_grad[0]:
            grad_input = input_grad_i4(grad_output, weight, scales, ctx.x_shape, ctx.x_dtype)
        return (grad_input,) + (None,) * (ctx.n_args - 1)


class W8A16MoeFunction(Function):
    """Autograd wrapper of the routed experts layer: forward = ``w8_a16_moe_train`` (the output bits of
    ``w8_a16_moe``), which also returns the routing tables, the gate|up projection and the per-slot down projection the backward
    reads; backward = ``w8_a16_moe_backward``: gradients of ``hidden_states`` and ``top_k_weights`` (the int8 stacks are frozen,
    the expert ids are integers).  The hidden states themselves are not saved."""

    @staticmethod
    def forward(ctx, hidden_states, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s):
        out, tables, gate_up, y = w8_a16_moe_train(hidden_states, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s)
        ctx.save_for_backward(top_k_weights, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        wts, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        grad_x, grad_w = w8_a16_moe_backward(grad_output, wts, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s, need_x, need_w)
        return grad_x, None, grad_w, None, None, None, None


class W4A16MoeFunction(Function):
    """:class:`W8A16MoeFunction` over int4 expert stacks: forward = ``w4_a16_moe_train`` on the module's ``path``
    (the output bits of ``w4_a16_moe`` on that path), backward = ``w4_a16_moe_backward``, whose two transposed grouped GEMMs read
    the int4 tiles themselves.  Gradients of ``hidden_states`` and ``top_k_weights`` only; the hidden states are not saved."""

    @staticmethod
    def forward(ctx, hidden_states, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s, path="auto"):
        out, tables, gate_up, y = w4_a16_moe_train(hidden_states, top_k_index, top_k_weights, gu_w, gu_s, dn_w, dn_s, path)
        ctx.save_for_backward(top_k_weights, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        wts, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        grad_x, grad_w = w4_a16_moe_backward(grad_output, wts, tables, gate_up, y, gu_w, gu_s, dn_w, dn_s, need_x, need_w)
        return grad_x, None, grad_w, None, None, None, None, None


class EetqLinear(nn.Module):
    """The module shape transformers/TGI instantiate: buffer ``weight`` int8 [in, out], ``weight_scales``
    registered later via :meth:`register_scale`, optional fp16 ``bias``."""

    def __init__(self, in_features, out_features, bias=True, device="cuda:0"):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.register_buffer("weight", torch.zeros((in_features, out_features), dtype=torch.int8, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros((out_features,), dtype=torch.float16, device=device))
        else:
            self.bias = None
        self.checkpoint_layout = None
        install_layout_hooks(self, "weight")

    def register(self, buffer_name, tensor):
        self.register_buffer(buffer_name, tensor)

    def register_scale(self, device):
        n = self.weight.shape[-1]
        self.register_buffer("weight_scales", torch.zeros((n,), dtype=torch.float16, device=device))

    def forward(self, input):
        if self.training:
            return EetqLinearMMFunction.apply(input, self.weight, self.weight_scales, self.bias)
        with torch.no_grad():
            return EetqLinearMMFunction.apply(input, self.weight, self.weight_scales, self.bias)
