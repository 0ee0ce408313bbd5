"""Whole-model quantisation entry point.

Host-side mirror of /root/reference/python/eetq/utils/quantizer.py:40-61 (``eet_quantize``) and the helpers
it needs from python/eetq/utils/base.py (``find_layers`` :280-285, ``set_op_by_name`` :25-38,
``get_named_linears`` :273-274).  The checkpoint-export helpers of base.py (fuse/split/"tp") are offline
weight surgery outside the GEMM path and are out of scope.
"""
import gc
import warnings

import torch
import torch.nn as nn

from ..modules.qlinear import EetqSparseMoeBlock, EetqTopKRouter, W4A16Experts, W4A16Linear, W8A16Experts, W8A16Linear

__all__ = ["eet_quantize", "find_layers", "set_op_by_name", "get_named_linears", "set_trainable", "set_prompt_path"]


def find_layers(module, include=(nn.Linear,), exclude=("lm_head",)):
    """name -> module for every submodule whose exact type is in ``include`` and whose qualified name
    contains none of the ``exclude`` substrings."""
    include = tuple(include)
    found = {}
    for name, sub in module.named_modules():
        if type(sub) in include and not any(tag in name for tag in exclude):
            found[name] = sub
    return found


def get_named_linears(module):
    return {name: m for name, m in module.named_modules() if isinstance(m, nn.Linear) and "lm_head" not in name}


def set_op_by_name(root, name, new_module):
    """Replace the submodule at dotted path ``name`` (numeric components index containers)."""
    *parents, leaf = name.split(".")
    node = root
    for part in parents:
        node = node[int(part)] if part.isdigit() else getattr(node, part)
    # plain assignment keeps the child's position in ordered containers (the reference's delattr + setattr moves
    # it to the end, which reorders an nn.Sequential)
    setattr(node, leaf, new_module)


def _progress(items, desc):
    try:
        from tqdm import tqdm
        return tqdm(items, desc=desc)
    except Exception:  # tqdm is cosmetic
        return items


def _experts_modules(model):
    """name -> module for every transformers-style experts module: 3-D ``gate_up_proj`` / ``down_proj`` parameters (or an
    ``up_proj`` stack for ungated experts), the layout MoE models keep their experts in since transformers 5."""
    found = {}
    for name, sub in model.named_modules():
        params = dict(sub.named_parameters(recurse=False))
        stacks = [params.get(n) for n in ("gate_up_proj", "up_proj", "down_proj")]
        if any(p is not None and p.dim() == 3 for p in stacks):
            found[name] = sub
    return found


def _swap_routers(model, quantised, exclude):
    """``router=True``: every allow-listed router becomes an :class:`EetqTopKRouter`, then every allow-listed block around quantised
    experts (``quantised``: their names) an :class:`EetqSparseMoeBlock`, both in place.  Returns one line per block of quantised
    experts whose router stays on torch."""
    for name, sub in list(model.named_modules()):
        if any(tag in name for tag in exclude):
            continue
        if type(sub).__name__ in EetqTopKRouter.CLASS_NAMES and EetqTopKRouter.unsupported_reason(sub) is None:
            EetqTopKRouter.from_router(sub)
    left = []
    for name in quantised:
        parent = name.rpartition(".")[0]
        block = model.get_submodule(parent) if parent else model
        gate = getattr(block, "gate", None)
        if not isinstance(gate, EetqTopKRouter):
            why = EetqTopKRouter.unsupported_reason(gate) if isinstance(gate, nn.Module) else "no gate module"
            left.append("%s (%s)" % (parent + ".gate" if parent else "gate", why))
        elif EetqSparseMoeBlock.unsupported_reason(block) is None:
            EetqSparseMoeBlock.from_block(block)
    return left


def set_trainable(model, flag=True, int4_experts=False):
    """Set the ``trainable`` flag of every :class:`W8A16Linear`, :class:`W4A16Linear` and :class:`W8A16Experts` in ``model``
    (itself included) -- with ``int4_experts=True`` of every :class:`W4A16Experts` as well -- and return how many modules it set.  Trainable modules pass gradients to their inputs (and, for experts, to
    the router weights) in grad mode; their quantised weights stay frozen and their output bits do not change.  Off by default: untrainable modules
    return detached outputs, as they always have.  Reversible: ``set_trainable(model, False)``.  Without ``int4_experts`` every
    :class:`W4A16Experts` is passed by and not counted, as before the int4 experts had a backward."""
    classes = (W8A16Linear, W4A16Linear, W8A16Experts) + ((W4A16Experts,) if int4_experts else ())
    n = 0
    for m in model.modules():
        if isinstance(m, classes):
            m.trainable = bool(flag)
            n += 1
    return n


def set_prompt_path(model, path):
    """Set ``prompt_path`` of every :class:`W4A16Linear` in ``model`` (itself included) and return how many modules it set:
    ``"direct"`` sends calls with more than 128 rows to the tiled kernel on the int4 tiles themselves where it takes the shape (no
    expansion to int8 tiles, no per-stream scratch, capturable into a graph cold), ``"auto"``, the default, leaves them on the
    expansion route (:class:`W4A16Linear`).  Any other value raises ValueError before a module is touched.  Int4
    experts have an attribute of their own (``eet_quantize(..., expert_prompt_path=...)``)."""
    if path not in W4A16Linear.PROMPT_PATHS:
        raise ValueError("set_prompt_path: path must be one of %r (got %r)" % (W4A16Linear.PROMPT_PATHS, path))
    n = 0
    for m in model.modules():
        if isinstance(m, W4A16Linear):
            m.prompt_path = path
            n += 1
    return n


def eet_quantize(model, init_only=False, include=[nn.Linear], exclude=["lm_head"], device="cuda:0", experts=False,
                 trainable=False, expert_bits=8, expert_prompt_path="auto", bits=8, router=False):
    """Swap every matching ``nn.Linear`` of ``model`` for a :class:`W8A16Linear` (in place).

    fp16 weights are quantised by the HIP quantiser; int8 weights (bitsandbytes ``Linear8bitLt``) reuse their
    ``SCB / 127`` scales; other dtypes raise ValueError.  ``device`` is accepted for signature
    compatibility; like the reference, each layer stays on the device its weight is on.
    ``experts=True`` (extension) also replaces every mixture-of-experts experts module that :class:`W8A16Experts` supports
    (3-D gated SiLU expert stacks: Mixtral, Qwen2/3-MoE, OLMoE, DeepSeek-V3 ...); unsupported ones stay as they are and are
    named in one warning.  The default leaves experts modules untouched.
    ``trainable=True`` (extension) then sets the flag of :func:`set_trainable` on every quantised module of the model, so that
    gradients cross them (fine-tuning adapters or prompts on a frozen int8 model).
    ``bits=4`` (extension) turns every fp16 target with ``in_features % 128 == 0`` and ``out_features % 16 == 0`` into a
    :class:`W4A16Linear` (int4 weights in the gfx950 int4 layout, half the bytes) instead; every other target -- a shape the int4
    layout does not hold, an int8 / bitsandbytes weight -- takes the int8 branch exactly as with ``bits=8``, and the fp16 targets
    left on int8 for their shape are named in one warning.  ``bits=4, trainable=True`` is allowed: :class:`W4A16Linear` has an
    input gradient (``w4_a16_gemm_t``).  Any value but 8 or 4 raises ValueError before the model is touched; the default changes
    nothing.
    ``expert_bits=4`` (extension; with ``experts=True``) builds :class:`W4A16Experts` -- int4 expert stacks, half the bytes,
    H and I multiples of 128 -- instead of :class:`W8A16Experts`; the ``nn.Linear`` pass stays int8.  Any value
    but 8 or 4, ``expert_bits=4`` without ``experts=True`` (it would quantise no expert and say nothing) and ``expert_bits=4``
    together with ``trainable=True`` raise ValueError before the model is touched: the int4 experts are made trainable afterwards,
    with ``set_trainable(model, True, int4_experts=True)``.
    ``expert_prompt_path="direct"`` (extension; with ``expert_bits=4``) sets :attr:`W4A16Experts.prompt_path` on every int4 experts
    module it builds: prompts then run the grouped tiled kernel on the int4 tiles instead of the decode kernel or the expansion
    (DESIGN.md 4.12).  The default ``"auto"`` changes nothing; any other value, or ``"direct"`` without ``expert_bits=4``, raises
    ValueError before the model is touched.
    ``router=True`` (extension; needs ``experts=True``, else ValueError before the model is touched) also moves the router onto
    the device kernel: every ``MixtralTopKRouter`` / ``Qwen2MoeTopKRouter`` / ``Qwen3MoeTopKRouter`` /
    ``OlmoeTopKRouter`` becomes an :class:`EetqTopKRouter`, and every ``MixtralSparseMoeBlock`` / ``Qwen3MoeSparseMoeBlock`` /
    ``OlmoeSparseMoeBlock`` whose experts were quantised an :class:`EetqSparseMoeBlock` (the whole block in four launches at
    T <= 16).  So do the sigmoid, bias-corrected, group-limited routers with DeepSeek-V3's forward --
    ``DeepseekV3TopkRouter`` / ``DeepseekV32TopkRouter`` / ``Glm4MoeTopkRouter`` / ``Glm4MoeLiteTopkRouter`` / ``Dots1TopkRouter`` /
    ``SolarOpenTopkRouter`` -- and the blocks around them, ``DeepseekV3MoE`` / ``DeepseekV32MoE`` / ``Glm4MoeMoE`` /
    ``Glm4MoeLiteMoE`` / ``Dots1MoE`` / ``SolarOpenMoE`` (the routed half in four launches, then the shared expert).  All are
    converted in place: parameters, buffers, state-dict keys and submodule names stay.  Other blocks (Qwen2-MoE's gated shared
    expert, other variants of bias-corrected routing, anything unknown) keep their block and get the router swap if their router is on
    the list; a quantised block whose router is not, or whose router's configuration the kernel does not serve, is named in the
    same warning as the experts left in fp16.
    """
    if isinstance(bits, bool) or not isinstance(bits, int) or bits not in (8, 4):
        raise ValueError("eet_quantize: bits must be 8 or 4 (got %r)" % (bits,))
    if expert_bits not in (8, 4):
        raise ValueError("eet_quantize: expert_bits must be 8 or 4 (got %r)" % (expert_bits,))
    if expert_bits == 4 and not experts:
        raise ValueError("eet_quantize: expert_bits=4 needs experts=True (without it no experts module is quantised)")
    if expert_bits == 4 and trainable:
        raise ValueError("eet_quantize: expert_bits=4 does not take trainable=True; quantise first, then make the int4 experts "
                         "trainable with set_trainable(model, True, int4_experts=True)")
    if expert_prompt_path not in W4A16Experts.PROMPT_PATHS:
        raise ValueError("eet_quantize: expert_prompt_path must be one of %r (got %r)" % (W4A16Experts.PROMPT_PATHS, expert_prompt_path))
    if expert_prompt_path != "auto" and expert_bits != 4:
        raise ValueError("eet_quantize: expert_prompt_path=%r needs expert_bits=4 (it is the int4 experts' switch)" % (expert_prompt_path,))
    if router and not experts:
        raise ValueError("eet_quantize: router=True needs experts=True (the device router feeds the quantised experts)")
    experts_cls = W4A16Experts if expert_bits == 4 else W8A16Experts
    if experts:
        skipped = []
        found = _experts_modules(model)
        quantised = []
        for name in list(found):
            mod = found.pop(name)  # the model and this loop hold the only references: the fp16 stacks go as each is replaced
            if any(tag in name for tag in exclude):
                continue
            why = experts_cls.unsupported_reason(mod)
            if why is not None:
                skipped.append("%s (%s)" % (name, why))
                continue
            qmod = experts_cls.from_experts(mod, init_only=init_only)
            if expert_prompt_path != "auto":
                qmod.prompt_path = expert_prompt_path
            set_op_by_name(model, name, qmod)
            quantised.append(name)
            del mod
            if not init_only and torch.cuda.is_available():
                torch.cuda.empty_cache()
        no_router = _swap_routers(model, quantised, exclude) if router else []
        if skipped or no_router:
            parts = []
            if skipped:
                parts.append("%d experts module(s) left in fp16: %s" % (len(skipped), "; ".join(skipped)))
            if no_router:
                parts.append("%d router(s) left on torch: %s" % (len(no_router), "; ".join(no_router)))
            warnings.warn("eet_quantize: " + ". ".join(parts))
    targets = find_layers(model, include=include, exclude=exclude)
    left_int8 = []
    desc = "[EET][INFO] quantization preprocessing..." + ("(init only)" if init_only else "")
    for name in _progress(list(targets), desc):
        linear = targets.pop(name)  # the model and this loop hold the only references
        wdtype = linear.weight.dtype
        if wdtype == torch.float16 and bits == 4 and linear.in_features % 128 == 0 and linear.out_features % 16 == 0:
            qlinear = W4A16Linear.from_torch(linear, init_only=init_only)
        elif wdtype == torch.float16:
            if bits == 4:
                left_int8.append("%s (%d -> %d)" % (name, linear.in_features, linear.out_features))
            qlinear = W8A16Linear.from_torch(linear, scales=None, init_only=init_only)
        elif wdtype == torch.int8:
            scales = torch.div(linear.state_dict()["SCB"], 127.0)
            qlinear = W8A16Linear.from_torch(linear, scales=scales, init_only=init_only)
        else:
            raise ValueError("Unsupported data type: {}".format(wdtype))
        set_op_by_name(model, name, qlinear)
        # the reference moves the replaced nn.Linear to the CPU before dropping it (quantizer.py:53-57): a 26 GB copy
        # over PCIe for a 13B model that nothing reads; dropping the last reference frees the HBM just the same
        del linear
        if not init_only and torch.cuda.is_available():
            torch.cuda.empty_cache()
    if left_int8:
        warnings.warn("eet_quantize: bits=4 needs in_features %% 128 == 0 and out_features %% 16 == 0; %d layer(s) quantised to "
                      "int8 instead: %s" % (len(left_int8), "; ".join(left_int8)))
    gc.collect()
    if trainable:
        set_trainable(model, True)
    return model
