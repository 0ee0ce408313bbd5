"""The operator module's own argument refusals for the mixture-of-experts ops (torch_ext.cpp: moe_rows_check, moe_stacks,
moe_routing_check, router_check, moe_plan and the backward's checks of its saved tensors): every condition, for every op that states
it, raises RuntimeError whose text starts with the op's name and holds the condition's wording -- and leaves nothing behind: the
same op called with valid arguments right after returns finite output.

E = 2, k = 1, H = I = 128, T = 2, zero stacks: a refusal happens before anything is launched, so the values do not matter."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, K, H, I, T = 2, 1, 128, 128, 2

LAYER = ("w8_a16_moe", "w8_a16_moe_train", "w4_a16_moe")
BLOCK = ("w8_a16_moe_block", "w4_a16_moe_block")
STACKED = LAYER + ("w8_a16_moe_backward",) + BLOCK
ROUTED = ("moe_router",) + BLOCK
STACK_NAMES = ("gate_up_qweight", "gate_up_scales", "down_qweight", "down_scales")


def _bits(op):
    return 4 if op.startswith("w4") else 8


def _rows(op):
    return "grad_out" if op == "w8_a16_moe_backward" else "hidden"


def _stacks(bits, h=H, i=I):
    pack = 2 if bits == 4 else 1
    shapes = ((E, h, 2 * i // pack), (E, 2 * i), (E, i, h // pack), (E, h))
    return {n: torch.zeros(s, dtype=torch.int8 if "qweight" in n else torch.float16, device=DEV) for n, s in zip(STACK_NAMES, shapes)}


@pytest.fixture(scope="module")
def saved():
    """what a valid w8_a16_moe_train call hands the backward: (tables, gate_up, y)"""
    from eetq_amd import ops
    return ops.w8_a16_moe_train(**_args("w8_a16_moe_train", None))[1:]


def _args(op, saved):
    """valid keyword arguments of `op`"""
    kw = {_rows(op): torch.randn(T, H, device=DEV).half()}
    if op in LAYER:
        kw.update(top_k_index=torch.zeros(T, K, dtype=torch.int64, device=DEV), top_k_weights=torch.ones(T, K, device=DEV))
    if op == "w8_a16_moe_backward":
        kw.update(top_k_weights=torch.ones(T, K, device=DEV), tables=saved[0], gate_up=saved[1], y=saved[2])
    if op in ROUTED:
        kw.update({"weight" if op == "moe_router" else "router_weight": torch.randn(E, H, device=DEV).half(), "top_k": K,
                   "norm_topk_prob": True, "scores_dtype": torch.float32})
    if op in STACKED:
        kw.update(_stacks(_bits(op)))
    return kw


def _set(name, make):
    """a mutation: argument `name` (None: the op's [T, H] argument, 'router': its router weight) becomes make(old value)"""
    def mutate(op, kw):
        key = {None: _rows(op), "router": "weight" if op == "moe_router" else "router_weight"}.get(name, name)
        kw[key] = make(kw[key])
    return mutate


def _other_h(h):   # hidden states, router weight and stacks all at another H
    def mutate(op, kw):
        kw[_rows(op)] = torch.randn(T, h, device=DEV).half()
        kw.update(_stacks(_bits(op), h))
        if op in BLOCK:
            kw["router_weight"] = torch.randn(E, h, device=DEV).half()
    return mutate


def _wider_hidden(op, kw):   # the hidden states (and, in front of the stacks' check, the router weight) at H = 256
    kw[_rows(op)] = torch.randn(T, 256, device=DEV).half()
    if op in BLOCK:
        kw["router_weight"] = torch.randn(E, 256, device=DEV).half()


def _strided(t):   # same shape, every other element of a buffer twice as wide
    return torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)[..., ::2]


def _grown(dim):
    def make(t):
        shape = list(t.shape)
        shape[dim] += 128
        return torch.zeros(shape, dtype=t.dtype, device=t.device)
    return make


# (ops, what is wrong, mutation, fragment of the message; {rows} is the op's [T, H] argument)
TABLE = [
    (LAYER + ROUTED + ("w8_a16_moe_backward",), "rows float32", _set(None, lambda t: t.float()), "{rows} must be a float16 GPU tensor [T, H]"),
    (LAYER + ROUTED + ("w8_a16_moe_backward",), "rows 3-D", _set(None, lambda t: t[None]), "{rows} must be a float16 GPU tensor [T, H]"),
    (LAYER + ROUTED + ("w8_a16_moe_backward",), "rows on the CPU", _set(None, lambda t: t.cpu()), "{rows} must be a float16 GPU tensor [T, H]"),
    (STACKED, "stack int16", _set("gate_up_qweight", lambda t: t.to(torch.int16)), "expert weights must be"),
    (STACKED, "scales float32", _set("down_scales", lambda t: t.float()), "expert weights must be"),
    (STACKED, "stack 2-D", _set("down_qweight", lambda t: t[0]), "expert weights must be"),
    (STACKED, "stacks differ in E", _set("down_qweight", _grown(0)), ": expected gate_up_"),
    (STACKED, "stacks differ in I", _set("down_qweight", _grown(1)), ": expected gate_up_"),
    (STACKED, "stacks differ in H", _set("down_scales", _grown(1)), ": expected gate_up_"),
    (STACKED, "stack not contiguous", _set("gate_up_qweight", _strided), "expert weights and scales must be contiguous"),
    (STACKED, "scales not contiguous", _set("down_scales", _strided), "expert weights and scales must be contiguous"),
    (STACKED, "stack on the CPU", _set("down_qweight", lambda t: t.cpu()), "all tensors must be on the hidden states' device"),
    (STACKED, "scales on the CPU", _set("gate_up_scales", lambda t: t.cpu()), "all tensors must be on the hidden states' device"),
    (("w8_a16_moe", "w8_a16_moe_train", "w8_a16_moe_backward", "w8_a16_moe_block"), "H = 96", _other_h(96),
     "the gfx950 layout needs H % 64 == 0 and I % 64 == 0"),
    (("w4_a16_moe", "w4_a16_moe_block"), "H = 192", _other_h(192), "the gfx950 int4 layout needs H % 128 == 0 and I % 128 == 0"),
    # the one wording this table does not take from the first version of these checks: the layer ops said "but gate_up_weight has H = "
    (STACKED, "H of the rows is not the stacks'", _wider_hidden, "{rows} is [T, 256] but the experts have H = 128"),
    (LAYER, "top_k_index [T + 1, k]", _set("top_k_index", lambda t: torch.zeros(T + 1, K, dtype=t.dtype, device=DEV)),
     "top_k_index and top_k_weights must both be [T, k]"),
    (LAYER, "top_k_weights [T, k + 1]", _set("top_k_weights", lambda t: torch.ones(T, K + 1, device=DEV)),
     "top_k_index and top_k_weights must both be [T, k]"),
    (LAYER + ("w8_a16_moe_backward",), "top_k_weights int32", _set("top_k_weights", lambda t: t.int()), "top_k_weights must be float32 or float16"),
    (LAYER, "top_k_index on the CPU", _set("top_k_index", lambda t: t.cpu()), "all tensors must be on the hidden states' device"),
    (ROUTED, "router weight float32", _set("router", lambda t: t.float()), "the router weight must be a float16 tensor [E, H] on the hidden states' device"),
    (ROUTED, "router weight on the CPU", _set("router", lambda t: t.cpu()), "the router weight must be a float16 tensor [E, H] on the hidden states' device"),
    (ROUTED, "router weight of another H", _set("router", lambda t: torch.zeros(E, 256, dtype=t.dtype, device=DEV)),
     "hidden is [T, 128] but the router weight has H = 256"),
    (BLOCK, "router weight of another E", _set("router", lambda t: torch.zeros(E + 1, H, dtype=t.dtype, device=DEV)),
     "the router weight has 3 experts but the stacks have E = 2"),
    (ROUTED, "top_k = 0", _set("top_k", lambda k: 0), "top_k must be in [1, E]"),
    (ROUTED, "top_k = E + 1", _set("top_k", lambda k: E + 1), "top_k must be in [1, E]"),
    (ROUTED, "scores_dtype bfloat16", _set("scores_dtype", lambda d: torch.bfloat16), "scores_dtype must be torch.float32 or torch.float16"),
    (("w4_a16_moe", "w4_a16_moe_block"), "path = 'fast'", lambda op, kw: kw.update(path="fast"), "path must be 'auto', 'decode' or 'expand'"),
    (("w4_a16_moe", "w4_a16_moe_block"), "path = 'expand' at H = I = 128", lambda op, kw: kw.update(path="expand"),
     "path='expand' needs a shape the grouped tiled kernel takes"),
    (("w8_a16_moe_backward",), "tables one short", _set("tables", lambda t: t[:-1].contiguous()),
     "tables must be w8_a16_moe_train's int32 routing tables for these T, k and E"),
    (("w8_a16_moe_backward",), "tables int64", _set("tables", lambda t: t.long()),
     "tables must be w8_a16_moe_train's int32 routing tables for these T, k and E"),
    (("w8_a16_moe_backward",), "gate_up [T k, I]", _set("gate_up", lambda t: t[:, :I].contiguous()),
     "gate_up must be w8_a16_moe_train's contiguous float16 [T*k, 2I]"),
    (("w8_a16_moe_backward",), "y not contiguous", _set("y", _strided), "y must be w8_a16_moe_train's contiguous float16 [T*k, H]"),
]
CASES = [pytest.param(op, mutate, text, id="%s-%s" % (op, what.replace(" ", "_"))) for ops, what, mutate, text in TABLE for op in ops]


@pytest.mark.parametrize("op,mutate,text", CASES)
def test_refusal_names_the_op_and_the_condition_and_leaves_nothing_behind(op, mutate, text, saved):
    from eetq_amd import ops
    fn = getattr(ops, op)
    kw = _args(op, saved)
    mutate(op, kw)
    with pytest.raises(RuntimeError) as err:
        fn(**kw)
    message = str(err.value)
    assert message.startswith(op + ": "), message
    assert text.format(rows=_rows(op)) in message, message
    out = fn(**_args(op, saved))
    torch.cuda.synchronize()
    for t in out if isinstance(out, tuple) else (out,):
        assert t is not None and bool(torch.isfinite(t.float()).all())
