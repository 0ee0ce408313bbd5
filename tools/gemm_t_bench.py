"""Time per call of the W8A16 input gradient at 7B / 13B shapes:
  (a) w8_a16_gemm_t(dy, W, s)                                        -- the fused op;
  (b) the identity path end to end: eye(K), w8_a16_gemm(eye, W, s) (dequantises W into fp16 [K, N]), dy @ W_deq^T in torch
      -- what EetqLinearMMFunction.backward ran before, and what transformers' shipped backward runs;
  (c) the forward w8_a16_gemm(x[M, K], W, s) at the same (M, K, N), for reference.
Event-timed loops after a warm-up (host launch time hidden behind the queue for every call that takes more than a few us),
plus the peak extra device memory one call of (a) and (b) allocates (its output included).  One JSON line per point on
stdout and in profiles/<tag>_gemm_t_bench.jsonl, stamped with the commit (EETQ_HEAD, passed in: the GPU box has no .git).

usage: EETQ_HEAD=$(git rev-parse --short HEAD) python tools/gemm_t_bench.py [--tag r07] [--rows 1,16,512,2048,4096]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from eetq_amd import ops  # noqa: E402

SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096), (5120, 13824), (13824, 5120)]   # (K, N) = (in, out)


def _head():
    h = os.environ.get("EETQ_HEAD")
    if h:
        return h
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE,
                               stderr=subprocess.DEVNULL, text=True, check=True).stdout.strip()
    except Exception:  # noqa: BLE001
        return "unknown"


def time_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def peak_extra_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    del out
    return extra / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r07")
    ap.add_argument("--rows", default="1,16,512,2048,4096")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    head = _head()
    out_path = os.path.join(ROOT, "profiles", "%s_gemm_t_bench.jsonl" % args.tag)
    lines = []
    for K, N in SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        w = ((torch.rand(K, N, device=dev, generator=g) * 2 - 1) / K ** 0.5).half()
        wq, s = ops.quant_weights(w, torch.int8, False)
        del w
        torch.cuda.empty_cache()
        for M in (int(r) for r in args.rows.split(",")):
            dy = torch.randn(M, N, device=dev, generator=g).half()
            x = torch.randn(M, K, device=dev, generator=g).half()

            def fused():
                return ops.w8_a16_gemm_t(dy, wq, s)

            def identity():
                eye = torch.eye(K, device=dev, dtype=torch.float16)
                w_deq = ops.w8_a16_gemm(eye, wq, s)
                return dy.matmul(w_deq.t())

            def forward():
                return ops.w8_a16_gemm(x, wq, s)

            iters = args.iters if M * N * K < 2 ** 36 else max(5, args.iters // 4)
            t_a = time_us(fused, args.warmup, iters)
            t_b = time_us(identity, args.warmup, max(3, iters // 2))
            t_c = time_us(forward, args.warmup, iters)
            rec = {"commit": head, "K": K, "N": N, "M": M, "gemm_t_us": round(t_a, 2), "identity_us": round(t_b, 2),
                   "forward_us": round(t_c, 2), "identity_over_gemm_t": round(t_b / t_a, 2),
                   "gemm_t_over_forward": round(t_a / t_c, 3), "gemm_t_TFLOPs": round(2 * M * N * K / t_a / 1e6, 1),
                   "gemm_t_extra_MiB": round(peak_extra_mib(fused), 2), "identity_extra_MiB": round(peak_extra_mib(identity), 2)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del dy, x
        del wq, s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
