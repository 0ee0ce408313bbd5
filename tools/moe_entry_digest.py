"""One call of every mixture-of-experts entry point of the operator module on seeded inputs, one line per call:

    op bits T path name=sha256(output bytes) ...

Every op is called twice -- a warm-up call, then the call whose outputs are hashed.  Two builds of eetq_amd/csrc/torch_ext.cpp that
print the same lines compute the same bits on every path the module can take: decode and tiled grouped kernels, the int4 expansion,
the quiet fall-back of a shape the tiled kernel refuses, the trainable forward and its backward, the device router below and above
T = 16, both block ops and, last, the sigmoid rule's router and block ops.  Under `rocprofv3 --kernel-trace --stats -- python tools/moe_entry_digest.py` the same run gives the
kernels each call launches.  Needs an MI355X.

    python tools/moe_entry_digest.py > digest.txt
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
E, K_TOP = 4, 2


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _stacks(bits, H, I, g):
    """any bytes are valid stacks: int8 [E, H, 2I] / [E, I, H], or int4 pairs [E, H, I] / [E, I, H / 2]"""
    pack = 2 if bits == 4 else 1
    lo = -128 if bits == 4 else -127
    gu_w = torch.randint(lo, 128, (E, H, 2 * I // pack), dtype=torch.int8, generator=g)
    dn_w = torch.randint(lo, 128, (E, I, H // pack), dtype=torch.int8, generator=g)
    amp = 2e-2 if bits == 4 else 1e-3
    gu_s = (torch.rand(E, 2 * I, generator=g) * amp).half()
    dn_s = (torch.rand(E, H, generator=g) * amp).half()
    return tuple(t.to(DEV) for t in (gu_w, gu_s, dn_w, dn_s))


def _inputs(T, H, g):
    x = torch.randn(T, H, generator=g).half().to(DEV)
    idx = torch.stack([torch.randperm(E, generator=g)[:K_TOP] for _ in range(T)]).to(DEV)
    wts = torch.rand(T, K_TOP, generator=g).softmax(-1).to(DEV)
    dout = torch.randn(T, H, generator=g).half().to(DEV)
    return x, idx, wts, dout


def _emit(op, bits, T, path, fn, names):
    fn()
    out = fn()
    torch.cuda.synchronize()
    out = out if isinstance(out, tuple) else (out,)
    assert len(out) == len(names), (op, len(out))
    for t in out:
        assert bool(torch.isfinite(t.float()).all()), op
    print(op, bits, T, path, " ".join("%s=%s" % (n, _sha(t)) for n, t in zip(names, out)), flush=True)


def main():
    assert torch.cuda.is_available(), "tools/moe_entry_digest.py needs a GPU"
    from eetq_amd import ops
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for H in (384, 256):   # 256: below the tiled kernel's K >= 320, so T = 40 falls back to the decode kernel quietly
            I = H
            s8, s4 = _stacks(8, H, I, g), _stacks(4, H, I, g)
            wr = (torch.randn(E, H, generator=g) / H ** 0.5).half().to(DEV)
            tag = "auto" if H == 384 else "auto/H=%d" % H
            for T in (3, 40) if H == 384 else (40,):
                x, idx, wts, dout = _inputs(T, H, g)
                _emit("w8_a16_moe", 8, T, tag, lambda: ops.w8_a16_moe(x, idx, wts, *s8), ["out"])

                def train_and_backward():
                    out, tables, gate_up, y = ops.w8_a16_moe_train(x, idx, wts, *s8)
                    gx, gw = ops.w8_a16_moe_backward(dout, wts, tables, gate_up, y, *s8, True, True)
                    return out, tables, gate_up, y, gx, gw
                _emit("w8_a16_moe_train+backward", 8, T, tag, train_and_backward, ["out", "tables", "gate_up", "y", "gx", "gw"])
                for dt in (torch.float32, torch.float16):
                    dtag = tag + "/" + str(dt).replace("torch.", "")
                    _emit("moe_router", "-", T, dtag, lambda: ops.moe_router(x, wr, K_TOP, True, dt), ["logits", "scores", "idx"])
                    _emit("w8_a16_moe_block", 8, T, dtag, lambda: ops.w8_a16_moe_block(x, wr, K_TOP, True, dt, *s8), ["out"])
                    _emit("w4_a16_moe_block", 4, T, dtag, lambda: ops.w4_a16_moe_block(x, wr, K_TOP, True, dt, *s4), ["out"])
            if H != 384:
                continue
            x, idx, wts, _ = _inputs(3, H, g)
            for path in ("auto", "decode", "expand"):
                _emit("w4_a16_moe", 4, 3, path, lambda: ops.w4_a16_moe(x, idx, wts, *s4, path=path), ["out"])
            # T k = 256 = 64 E: the first shape the measured rule sends to the expanded path
            assert ops.w4_a16_moe_path(128, K_TOP, E, H, I) == "expand"
            assert ops.w4_a16_moe_path(127, K_TOP, E, H, I) == "decode"
            x, idx, wts, _ = _inputs(128, H, g)
            _emit("w4_a16_moe", 4, 128, "auto", lambda: ops.w4_a16_moe(x, idx, wts, *s4), ["out"])
        # the sigmoid, group-limited rule, drawn after everything above: 2 groups of 2 experts, 1 kept
        H = I = 384
        s8, s4 = _stacks(8, H, I, g), _stacks(4, H, I, g)
        wr = (torch.randn(E, H, generator=g) / H ** 0.5).half().to(DEV)
        bias = (torch.rand(E, generator=g) * 0.5 - 0.25).half().to(DEV)
        rule = (bias, K_TOP, 2, 1, True, 2.5)
        for T in (3, 40):
            x = _inputs(T, H, g)[0]
            _emit("moe_router_sigmoid", "-", T, "auto", lambda: ops.moe_router_sigmoid(x, wr, *rule), ["logits", "weights", "idx"])
            _emit("w8_a16_moe_block_sigmoid", 8, T, "auto", lambda: ops.w8_a16_moe_block_sigmoid(x, wr, *rule, *s8), ["out"])
            _emit("w4_a16_moe_block_sigmoid", 4, T, "auto", lambda: ops.w4_a16_moe_block_sigmoid(x, wr, *rule, *s4), ["out"])


if __name__ == "__main__":
    main()
