"""Time one W8A16 mixture-of-experts layer (ops.w8_a16_moe) on synthetic routing; one JSON line per (shape, T, routing).

Columns: us per layer (median of --iters launches after --warmup), int8 bytes of the active experts / us, transformers' eager fp16
experts forward (MixtralExperts) on the same routing, and a Python loop of per-expert w8_a16_gemm calls (gather, gate|up with
silu_glu8, down, weighted index_add).  Weights are random (int8 stacks, small fp16 scales): the time depends on shapes only.

    python tools/moe_bench.py --out profiles/r07_moe_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"mixtral-8x7b": (4096, 14336, 8, 2), "qwen3-30b-a3b": (2048, 768, 128, 8)}
DEV = "cuda:0"


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return times[len(times) // 2]


def _routing(T, k, E, kind, g):
    if kind == "uniform":
        return torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(DEV)
    # skewed: every token's first choice is expert 0
    rest = torch.stack([torch.randperm(E - 1, generator=g)[:k - 1] + 1 for _ in range(T)])
    return torch.cat([torch.zeros(T, 1, dtype=torch.long), rest], 1).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--tokens", default="1,2,4,8,16,64,512")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd.ops import w8_a16_gemm, w8_a16_moe
    out = open(args.out, "w") if args.out else None
    for name in args.shapes.split(","):
        H, I, E, k = SHAPES[name]
        torch.manual_seed(0)
        gu_w = torch.randint(-127, 128, (E, H, 2 * I), dtype=torch.int8, device=DEV)
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-3).half()
        dn_w = torch.randint(-127, 128, (E, I, H), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-3).half()
        cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)
        cfg._experts_implementation = "eager"
        eager = MixtralExperts(cfg).half().to(DEV)
        with torch.no_grad():
            eager.gate_up_proj.normal_(0, 0.02)
            eager.down_proj.normal_(0, 0.02)
        g = torch.Generator().manual_seed(1)
        for T in (int(t) for t in args.tokens.split(",")):
            for kind in ("uniform", "skewed"):
                x = (torch.rand(T, H, device=DEV) - 0.5).half()
                idx = _routing(T, k, E, kind, g)
                wts = torch.rand(T, k, device=DEV).softmax(-1)
                active = torch.unique(idx).tolist()

                def loop():
                    y = torch.zeros(T, H, dtype=torch.float16, device=DEV)
                    for e in active:
                        tok, j = torch.where(idx == e)
                        h = w8_a16_gemm(x.index_select(0, tok), gu_w[e], gu_s[e], activation="silu_glu8")
                        d = w8_a16_gemm(h, dn_w[e], dn_s[e])
                        y.index_add_(0, tok, d * wts[tok, j, None].half())
                    return y

                us = _time(lambda: w8_a16_moe(x, idx, wts, gu_w, gu_s, dn_w, dn_s), args.warmup, args.iters)
                with torch.no_grad():
                    us_eager = _time(lambda: eager(x, idx, wts), args.warmup, args.iters)
                us_loop = _time(loop, args.warmup, args.iters)
                nbytes = len(active) * 3 * H * I
                rec = {"shape": name, "H": H, "I": I, "E": E, "k": k, "T": T, "routing": kind, "active_experts": len(active),
                       "path": "device" if T <= 16 else "host", "us": round(us, 2), "int8_bytes": nbytes,
                       "TBps": round(nbytes / us / 1e6, 3), "us_fp16_eager": round(us_eager, 2),
                       "us_per_expert_loop": round(us_loop, 2), "speedup_vs_eager": round(us_eager / us, 2)}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
