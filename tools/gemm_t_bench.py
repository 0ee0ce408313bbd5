"""Time per call of the W8A16 input gradient at 7B / 13B shapes:
  (a) w8_a16_gemm_t(dy, W, s)                                        -- the fused op;
  (b) the identity path end to end: eye(K), w8_a16_gemm(eye, W, s) (dequantises W into fp16 [K, N]), dy @ W_deq^T in torch
      -- what EetqLinearMMFunction.backward ran before, and what transformers' shipped backward runs;
  (c) the forward w8_a16_gemm(x[M, K], W, s) at the same (M, K, N), for reference.
Event-timed loops after a warm-up (host launch time hidden behind the queue for every call that takes more than a few us),
plus the peak extra device memory one call of (a) and (b) allocates (its output included).  One JSON line per point on
stdout and in profiles/<tag>_gemm_t_bench.jsonl, stamped with the commit (EETQ_HEAD, passed in: the GPU box has no .git).

usage: EETQ_HEAD=$(git rev-parse --short HEAD) python tools/gemm_t_bench.py [--tag r07] [--rows 1,16,512,2048,4096]

--bits 4 times the int4 input gradient instead (profiles/<tag>_gemm_t_int4_bench.jsonl), K x N in 4096^2, 4096 x 11008,
11008 x 4096 and M in 16, 512, 2048 by default, on random int4 values held both as int4 and as int8 tiles:
  (a) w4_a16_gemm_t(dy, W4, s);
  (b) w8_a16_gemm_t(dy, W8, s) on the same integers -- same tile, same MFMA and LDS work, twice the weight bytes;
  (c) the int4 identity path end to end: eye(K), w8_a16_gemm(eye, W4, s), dy @ W_deq^T in torch.
--repeats (default 3) timed loops per point, each kept: the spread between repeats is what a difference between (a) and (b)
has to exceed to mean anything.
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


def main_int4(args, dev, head):
    out_path = os.path.join(ROOT, "profiles", "%s_gemm_t_int4_bench.jsonl" % args.tag)
    rows = [int(r) for r in (args.rows or "16,512,2048").split(",")]
    lines = []
    for K, N in SHAPES[:3]:
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        q = torch.randint(-8, 8, (K, N), device=dev, generator=g, dtype=torch.int8)
        s = (torch.rand(N, device=dev, generator=g) * 0.02 + 1e-3).half()
        w8 = ops.preprocess_weights(q)
        # raw int4 [K, N / 2]: byte j of a row = column 2 j in the low nibble, column 2 j + 1 in the high one
        w4 = ops.preprocess_weights(((q[:, 0::2] & 0xF) | (q[:, 1::2] << 4)).contiguous(), True)
        del q
        torch.cuda.empty_cache()
        for M in rows:
            dy = torch.randn(M, N, device=dev, generator=g).half()

            def int4():
                return ops.w4_a16_gemm_t(dy, w4, s)

            def int8():
                return ops.w8_a16_gemm_t(dy, w8, s)

            def identity():
                eye = torch.eye(K, device=dev, dtype=torch.float16)
                w_deq = ops.w8_a16_gemm(eye, w4, s)
                return dy.matmul(w_deq.t())

            assert torch.equal(int4(), int8())
            iters = args.iters if M * N * K < 2 ** 36 else max(5, args.iters // 4)
            t_a, t_b, t_c = [], [], []
            for _ in range(args.repeats):   # interleaved, so a drift of the clocks hits the three columns alike
                t_a.append(round(time_us(int4, args.warmup, iters), 2))
                t_b.append(round(time_us(int8, args.warmup, iters), 2))
                t_c.append(round(time_us(identity, args.warmup, max(3, iters // 2)), 2))
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            rec = {"commit": head, "K": K, "N": N, "M": M, "int4_gemm_t_us": t_a, "int8_gemm_t_us": t_b, "int4_identity_us": t_c,
                   "int4_over_int8": round(med(t_a) / med(t_b), 3), "identity_over_int4": round(med(t_c) / med(t_a), 2),
                   "int4_TFLOPs": round(2 * M * N * K / med(t_a) / 1e6, 1),
                   "int4_extra_MiB": round(peak_extra_mib(int4), 2), "identity_extra_MiB": round(peak_extra_mib(identity), 2),
                   "three_KN_MiB": round(3 * K * N / 2 ** 20, 2)}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del dy
        del w4, w8, s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r07")
    ap.add_argument("--rows", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bits", type=int, default=8, choices=(8, 4))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    head = _head()
    if args.bits == 4:
        return main_int4(args, dev, head)
    args.rows = args.rows or "1,16,512,2048,4096"
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
