"""Few-row attention behind a long cache (ops.decode_attention_rows, eetq_decode_attention_rows_f16) against the path a verify step
took before it -- ops.prefill_attention(kv_len=counter) at its default splits, the comparand -- and against the one-row decode
attention (ops.decode_attention), the floor.  Heads 40 x 128 (MHA) and 32 / 8 x 128; R in {3, 5, 9, 16} rows behind 1 024, 4 096 and
16 384 cached rows; batch 1 and 4.

Per point: microseconds per call of --calls dependent launches (one stream, each call behind the one before it) captured as ONE
graph and replayed, the median of --reps device-event timings (the first timing warms up and is dropped); the rows op at the rule's
chunk count and at forced counts (the table the rule is tuned from); the largest absolute difference of the rows op from a float32
softmax(q k^T) v of the same inputs, and from the prompt kernel.  Writes every point to --out (default profiles/attn_rows.txt).
usage: python tools/attn_rows_bench.py [--calls 10] [--reps 9] [--quick]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import eetq_amd.ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--quick", action="store_true", help="one geometry, two caches: a look, not the table")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_rows.txt"))
args = ap.parse_args()
DEV = "cuda:0"
FORCED = (2, 4, 8, 16, 32, 64)


def graph_us(step):
    """median microseconds per call: args.calls back-to-back calls in one captured graph, args.reps + 1 timed replays"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(args.calls):
            step()
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(args.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(8):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / (8 * args.calls))
    return statistics.median(us[1:])


def reference(q, kc, vc, keys):
    B, R, H, D = q.shape
    Hkv = kc.shape[1]
    k, v = kc[:, :, :keys].float(), vc[:, :, :keys].float()
    if Hkv != H:
        k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    sc = torch.matmul(q.transpose(1, 2).float(), k.transpose(2, 3)) / D ** 0.5
    mask = torch.arange(keys, device=DEV)[None, :] > (torch.arange(R, device=DEV)[:, None] + keys - R)
    return torch.matmul(torch.softmax(sc.masked_fill(mask, float("-inf")), -1), v).transpose(1, 2)


def main():
    assert torch.cuda.is_available() and ops.decode_attention_rows is not None, "needs a GPU and the compiled operator module"
    D, pad = 128, 16
    geos = ((40, 40),) if args.quick else ((40, 40), (32, 8))
    caches = (1024, 4096) if args.quick else (1024, 4096, 16384)
    lines = ["# tools/attn_rows_bench.py on %s: us per call, median of %d timings of 8 replays of a graph of %d dependent calls"
             % (torch.cuda.get_device_name(0), args.reps, args.calls),
             "# prompt = ops.prefill_attention(kv_len=counter) at its default splits (the verify step's path before this kernel);",
             "# decode1 = ops.decode_attention on one row (the floor); rows = ops.decode_attention_rows at the rule's chunk count;",
             "# sN = rows at N forced chunks; err = max |rows - float32 reference|, vs_prompt = max |rows - prompt|",
             "%7s %2s %3s %6s | %8s %8s %8s %5s | %s | %8s %9s" % ("H/Hkv", "B", "R", "cached", "prompt", "decode1", "rows", "rule",
                                                                " ".join("%7s" % ("s%d" % n) for n in FORCED), "err", "vs_prompt")]
    print("\n".join(lines), flush=True)
    torch.manual_seed(0)
    for H, Hkv in geos:
        for B in (1, 4):
            for cached in caches:
                for R in (3, 5, 9, 16):
                    keys = cached + R
                    qkv = torch.randn(B, R, (H + 2 * Hkv) * D, dtype=torch.float16, device=DEV)
                    q = qkv[..., :H * D].unflatten(-1, (H, D))
                    kc = torch.randn(B, Hkv, keys + pad, D, dtype=torch.float16, device=DEV)
                    vc = torch.randn(B, Hkv, keys + pad, D, dtype=torch.float16, device=DEV)
                    n = torch.tensor([keys], dtype=torch.int64, device=DEV)
                    rule = ops.decode_attention_rows_splits(B, H, Hkv, R, keys + pad)
                    ws = torch.empty(B * H * R * 64 * (D + 4), dtype=torch.float32, device=DEV)
                    q1 = q[:, 0]
                    t_prompt = graph_us(lambda: ops.prefill_attention(q, kc, vc, keys + pad, kv_len=n))
                    t_dec = graph_us(lambda: ops.decode_attention(q1, kc, vc, kv_len=n))
                    t_rows = graph_us(lambda: ops.decode_attention_rows(q, kc, vc, keys + pad, kv_len=n, workspace=ws))
                    forced = [graph_us(lambda ns=ns: ops.decode_attention_rows(q, kc, vc, keys + pad, kv_len=n, splits=ns, workspace=ws))
                              for ns in FORCED]
                    out = ops.decode_attention_rows(q, kc, vc, keys + pad, kv_len=n).float()
                    err = (out - reference(q, kc, vc, keys)).abs().max().item()
                    vs = (out - ops.prefill_attention(q, kc, vc, keys + pad, kv_len=n).float()).abs().max().item()
                    line = "%4d/%-2d %2d %3d %6d | %8.1f %8.1f %8.1f %5d | %s | %8.5f %9.5f" % (
                        H, Hkv, B, R, cached, t_prompt, t_dec, t_rows, rule, " ".join("%7.1f" % t for t in forced), err, vs)
                    print(line, flush=True)
                    lines.append(line)
                    del qkv, kc, vc, ws
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
