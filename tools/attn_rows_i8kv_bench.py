"""Few-row attention behind INT8 cache rows (ops.decode_attention_rows_i8kv, eetq_decode_attention_rows_i8kv_f16) against the route a
"prompt" verify step takes on an int8 cache -- ops.prefill_attention_i8kv(kv_len=counter) at its default splits, the comparand -- and
against the fp16 few-row kernel (ops.decode_attention_rows) on fp16 rows of the same values.  The method and the points are
tools/attn_rows_bench.py's: heads 40 x 128 (MHA) and 32 / 8 x 128; R in {3, 5, 9, 16} rows behind 1 024, 4 096 and 16 384 cached rows;
batch 1 and 4.

Per point: microseconds per call of --calls dependent launches (one stream, each call behind the one before it) captured as ONE
graph and replayed, the median of --reps device-event timings (the first timing warms up and is dropped); the int8 rows op at the
rule's chunk count (eetq_decode_attention_rows_splits: tuned on fp16 rows, reused untuned) and at forced counts; `model` = the fp16
rows time x (2 D + 4) / (4 D), the bytes a row costs in either cache -- what the int8 call would approach if it were bound by the
cache stream alone; the largest absolute difference of the int8 rows op from a float32 softmax(q k^T) v on the dequantised rows, and
from the int8 prompt kernel.  Writes every point to --out (default profiles/attn_rows_i8kv.txt).
usage: python tools/attn_rows_i8kv_bench.py [--calls 10] [--reps 9] [--quick]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_rows_i8kv.txt"))
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


def quantize(x):
    """fp16 rows [B, Hkv, S, D] -> int8 bytes and fp16 scales [B, Hkv, S] in the row format of the cache (amax / 127, round half away)"""
    s = (x.float().abs().amax(-1) * (1.0 / 127.0)).half()
    y = x.float() / s.float().clamp_min(1e-30)[..., None]
    q = torch.where(y < 0, torch.ceil(y - 0.5), torch.floor(y + 0.5)).clamp_(-127, 127)
    return q.to(torch.int8), s


def reference(q, kd, vd, keys):
    B, R, H, D = q.shape
    Hkv = kd.shape[1]
    k, v = kd[:, :, :keys], vd[:, :, :keys]
    if Hkv != H:
        k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    sc = torch.matmul(q.transpose(1, 2).float(), k.transpose(2, 3)) / D ** 0.5
    mask = torch.arange(keys, device=DEV)[None, :] > (torch.arange(R, device=DEV)[:, None] + keys - R)
    return torch.matmul(torch.softmax(sc.masked_fill(mask, float("-inf")), -1), v).transpose(1, 2)


def main():
    assert torch.cuda.is_available() and ops.decode_attention_rows_i8kv is not None, "needs a GPU and the compiled operator module"
    D, pad = 128, 16
    geos = ((40, 40),) if args.quick else ((40, 40), (32, 8))
    caches = (1024, 4096) if args.quick else (1024, 4096, 16384)
    lines = ["# tools/attn_rows_i8kv_bench.py on %s: us per call, median of %d timings of 8 replays of a graph of %d dependent calls"
             % (torch.cuda.get_device_name(0), args.reps, args.calls),
             "# prompt8 = ops.prefill_attention_i8kv(kv_len=counter) at its default splits (a \"prompt\" verify step on an int8 cache);",
             "# rows16 = ops.decode_attention_rows on fp16 rows at the rule's chunk count; model = rows16 x (2 D + 4) / (4 D);",
             "# rows8 = ops.decode_attention_rows_i8kv at the rule's chunk count (the fp16 rule, untuned); sN = rows8 at N forced chunks;",
             "# err = max |rows8 - float32 reference on the dequantised rows|, vs_prompt = max |rows8 - prompt8|",
             "%7s %2s %3s %6s | %8s %8s %8s %8s %5s | %s | %8s %9s" % ("H/Hkv", "B", "R", "cached", "prompt8", "rows16", "model", "rows8", "rule",
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
                    (k8, ks), (v8, vs) = quantize(kc), quantize(vc)
                    sc = torch.stack([ks, vs], dim=-1).contiguous()
                    n = torch.tensor([keys], dtype=torch.int64, device=DEV)
                    rule = ops.decode_attention_rows_splits(B, H, Hkv, R, keys + pad)
                    ws = torch.empty(B * H * R * 64 * (D + 4), dtype=torch.float32, device=DEV)
                    t_prompt = graph_us(lambda: ops.prefill_attention_i8kv(q, k8, v8, sc, keys + pad, kv_len=n))
                    t_16 = graph_us(lambda: ops.decode_attention_rows(q, kc, vc, keys + pad, kv_len=n, workspace=ws))
                    t_rows = graph_us(lambda: ops.decode_attention_rows_i8kv(q, k8, v8, sc, keys + pad, kv_len=n, workspace=ws))
                    forced = [graph_us(lambda ns=ns: ops.decode_attention_rows_i8kv(q, k8, v8, sc, keys + pad, kv_len=n, splits=ns,
                                                                                   workspace=ws)) for ns in FORCED]
                    out = ops.decode_attention_rows_i8kv(q, k8, v8, sc, keys + pad, kv_len=n).float()
                    kd, vd = k8.float() * ks.float()[..., None], v8.float() * vs.float()[..., None]
                    err = (out - reference(q, kd, vd, keys)).abs().max().item()
                    vs_p = (out - ops.prefill_attention_i8kv(q, k8, v8, sc, keys + pad, kv_len=n).float()).abs().max().item()
                    line = "%4d/%-2d %2d %3d %6d | %8.1f %8.1f %8.1f %8.1f %5d | %s | %8.5f %9.5f" % (
                        H, Hkv, B, R, cached, t_prompt, t_16, t_16 * (2 * D + 4) / (4 * D), t_rows, rule,
                        " ".join("%7.1f" % t for t in forced), err, vs_p)
                    print(line, flush=True)
                    lines.append(line)
                    del qkv, kc, vc, k8, v8, sc, kd, vd, ws
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
