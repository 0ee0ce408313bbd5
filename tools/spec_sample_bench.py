"""The sampled verify step's hand-over (ops.spec_sample_accept), timed as tools/sample_bench.py times the plain
one: a chain of L dependent launches on the same counters inside one HIP graph, microseconds per launch, median [min, max] of
the replays.  For V in {32000, 128256} x B in {1, 4} x k in {4, 8}, at T = 0, T = 0.8 + top-k 50 and T = 0.8 + top-k 50 + top-p 0.9,
with the draft fully accepted and with the draft rejected at position 0 (the random numbers are served, so that a draft can be
right at every column of the chain), next to
  (i)  ops.spec_accept on the same logits and drafts (the greedy walk: one workgroup, rows in series),
  (ii) one ops.sample_handover launch on B rows -- the serial work the new launch replaces is (k + 1) x (ii).
Writes the table to --out (default profiles/spec_sample_accept.txt) and exits non-zero if any point is not below (k + 1) x (ii).
usage: python tools/spec_sample_bench.py [--chain 32] [--reps 20]"""
import argparse
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_sample_accept.txt"))
args = ap.parse_args()
dev = "cuda:0"
L = args.chain
SETTINGS = [("T=0", dict(temperature=0.0)), ("top-k 50", dict(temperature=0.8, top_k=50)),
            ("top-k 50 + top-p 0.9", dict(temperature=0.8, top_k=50, top_p=0.9))]


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


def fmt(t):
    return "%7.1f [%6.1f, %6.1f]" % t


def main():
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=dev)
    lines = ["us per launch, median [min, max] of %d replays of a graph of %d dependent launches" % (args.reps, L),
             "%6s %2s %2s  %-21s %-8s  %-24s %-24s %-24s %6s %6s" % ("V", "B", "k", "setting", "draft", "spec_sample_accept",
                                                                    "(i) spec_accept", "(ii) sample_handover", "/(ii)", "/(k+1)(ii)")]
    worst = 0.0
    for V in (32000, 128256):
        for B in (1, 4):
            for k in (4, 8):
                torch.manual_seed(V + B + k)
                lg = (torch.randn(B, k + 1, V, device=dev) * 3).half()
                uni = torch.rand(B, k + 1, device=dev)
                out, col, tok, pos = i64(B, 64), i64(1, 1), i64(B, 1), i64(1)
                limit, hist, stats = torch.full((1,), 1 << 38, dtype=torch.int64, device=dev), i64(B, 64), i64(2)
                done, ws = torch.zeros(B, dtype=torch.int32, device=dev), i64(B * (k + 1))
                for name, kw in SETTINGS:
                    params = ops.sampling_params(device=dev, **kw)
                    base = timed(lambda: ops.sample_handover(lg[:, 0], out, col, tok, pos, params, done))
                    # the tokens of the served numbers: sample_handover per position (the contract's words)
                    x = i64(B, k + 1)
                    for t in range(k + 1):
                        ops.sample_handover(lg[:, t], out, col, tok, pos, params, done, uni[:, t].contiguous())
                        x[:, t:t + 1] = tok
                    g = lg.argmax(-1)
                    for what in ("accepted", "rejected"):
                        draft, gdraft = x[:, :k].clone(), g[:, :k].clone()
                        if what == "rejected":
                            draft[:, 0] = (draft[:, 0] + 1) % V
                            gdraft[:, 0] = (gdraft[:, 0] + 1) % V
                        col.zero_(); pos.zero_(); stats.zero_()
                        new = timed(lambda: ops.spec_sample_accept(lg, draft, out, col, tok, pos, limit, hist, stats, params, done, uni, ws))
                        steps, tokens = stats.tolist()
                        assert tokens == steps * (k + 1 if what == "accepted" else 1), (what, steps, tokens)
                        col.zero_(); pos.zero_(); stats.zero_()
                        old = timed(lambda: ops.spec_accept(lg, gdraft, out, col, tok, pos, limit, hist, stats))
                        ratio = new[0] / base[0]
                        worst = max(worst, ratio / (k + 1))
                        lines.append("%6d %2d %2d  %-21s %-8s  %s %s %s %6.2f %6.2f" % (V, B, k, name, what, fmt(new), fmt(old), fmt(base),
                                                                                     ratio, ratio / (k + 1)))
                        print(lines[-1], flush=True)
    lines.append("worst spec_sample_accept / ((k + 1) x (ii)): %.2f (must stay below 1)" % worst)
    print(lines[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if worst < 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
