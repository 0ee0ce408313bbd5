"""The decode step's token hand-over, timed as the graph decoder issues it: a chain of L dependent launches on the same
counters inside one HIP graph (every launch waits for the one before it, like the steps of a decode graph).
Prints microseconds per launch (median of 20 replays, min, max) for V in {32000, 128256} x B in {1, 4} of
  (a) ops.greedy_handover, (b) ops.sample_handover at temperature 0, (c) temperature 0.8 + top-k 50, (d) temperature 0.8 +
  top-p 0.9, (e) both filters, (f) the torch chain a user would otherwise capture: divide, TopKLogitsWarper, TopPLogitsWarper,
  softmax, multinomial, scatter_, copy_, two add_
and writes one JSON line per row to --out (default profiles/sample_handover_bench.jsonl).
usage: python tools/sample_bench.py [--chain 32] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eetq_amd.ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chain", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_handover_bench.jsonl"))
args = ap.parse_args()
dev = "cuda:0"
L = args.chain


def timed(fn):
    """median, min, max microseconds per launch over args.reps replays of a graph of L chained calls"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(L):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / L)
    return statistics.median(us), min(us), max(us)


def main():
    from transformers.generation.logits_process import TopKLogitsWarper, TopPLogitsWarper
    rows = []
    for V in (32000, 128256):
        for B in (1, 4):
            torch.manual_seed(V + B)
            lg = (torch.randn(B, V, device=dev) * 3).half()
            out = torch.zeros(B, (args.reps + 8) * L + 64, dtype=torch.int64, device=dev)   # every launch of a case has its column
            col = torch.zeros(1, 1, dtype=torch.int64, device=dev)
            tok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
            pos = torch.zeros(1, dtype=torch.int64, device=dev)
            done = torch.zeros(B, dtype=torch.int32, device=dev)
            blocks = {"b_sample_t0": ops.sampling_params(temperature=0.0, device=dev),
                      "c_topk50": ops.sampling_params(temperature=0.8, top_k=50, device=dev),
                      "d_topp0.9": ops.sampling_params(temperature=0.8, top_p=0.9, device=dev),
                      "e_topk50_topp0.9": ops.sampling_params(temperature=0.8, top_k=50, top_p=0.9, device=dev)}
            topk, topp = TopKLogitsWarper(50), TopPLogitsWarper(0.9)

            def torch_chain(k=True, p=True):
                s = lg.float() / 0.8
                if k:
                    s = topk(None, s)
                if p:
                    s = topp(None, s)
                nxt = torch.multinomial(torch.softmax(s, -1), 1)
                out.scatter_(1, col.expand(B, 1), nxt)
                tok.copy_(nxt)
                pos.add_(1)
                col.add_(1)

            res = {"V": V, "B": B, "chain": L, "reps": args.reps, "unit": "us per launch: median, min, max"}
            cases = [("a_greedy", lambda: ops.greedy_handover(lg, out, col, tok, pos))]
            cases += [(n, (lambda blk: lambda: ops.sample_handover(lg, out, col, tok, pos, blk, done))(blk))
                      for n, blk in blocks.items()]
            cases += [("f_torch_topk50", lambda: torch_chain(True, False)), ("f_torch_topp0.9", lambda: torch_chain(False, True)),
                      ("f_torch_topk50_topp0.9", lambda: torch_chain(True, True))]
            for name, fn in cases:
                col.zero_()
                res[name] = [round(x, 2) for x in timed(fn)]
            print(json.dumps(res), flush=True)
            rows.append(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
