"""Time per call of the W4A16 GEMV / GEMM next to W8A16 on the same shapes: HIP-graph-replayed chains of back-to-back calls
over rotating weight sets (tools/sweep.py::chain_us) -- NOT start/stop event pairs, whose ~4.2 us floor made the round-2
table read 4.3 us for both at 4096^2.

  python tools/int4_bench.py [M,M,...]              W4A16 AUTO next to W8A16 AUTO (the table above)
  python tools/int4_bench.py --prompt [M,M,...]     prompts on an int4 weight: the expansion route,
      w8_a16_gemm(x, w4, s, path="mfma"), against the tile on the int4 tiles themselves, w4_a16_gemm_tiled(x, w4, s) -- 7B and 13B
      projections, M = 129 .. 4096.  One JSON line per point, also appended to profiles/int4_prompt_direct.jsonl: both times (us per
      call, the better of two alternating runs, and each run), the tile shapes the direct launcher takes, the W8A16 AUTO path the
      expansion route ends in (eetq_diag_auto_path: path 6 with detail S > 1 slices K, and the bits may then differ), and
      torch.equal of the two outputs."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from eetq_amd import ops
from sweep import chain_us

dev = "cuda:0"
SHAPES = [(4096, 4096), (4096, 11008), (11008, 4096), (5120, 5120), (5120, 13824), (13824, 5120)]


def direct_plan(M, N, K, n_cu):
    """launch_gemm_tile_i4's plan at tile_j = 0 (eetq_diag_tile_plan: the planner the launcher walks): the tile shapes of its one
    or two launches"""
    import ctypes
    from eetq_amd import _lib
    rec, count = (ctypes.c_int * 12)(), ctypes.c_int(0)
    _lib.check(_lib.lib().eetq_diag_tile_plan(4, M, N, K, 0, 0, n_cu, rec, 2, ctypes.byref(count)))
    assert count.value <= 2, "more than one row chunk"
    shapes = ["128x64" if rec[6 * i + 4] == 1 else "128x128" for i in range(count.value)]
    return shapes[0] if count.value == 1 else "%s[:%d]+%s" % (shapes[0], rec[3], shapes[1])


def chain_on(stream, step, calls):
    """tools/sweep.py::chain_us on ONE caller-owned stream: warm-up and capture share it, so the per-stream expansion scratch the
    eager warm-up creates is the one the captured launches use (it cannot grow during capture)"""
    import time
    with torch.cuda.stream(stream):
        for i in range(2):
            step(i)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for i in range(calls):
                step(i)
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.replay()
    torch.cuda.synchronize()
    reps = max(2, int(0.05 / max(time.perf_counter() - t0, 1e-6)))
    best = 1e30
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            g.replay()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / (reps * calls))
    del g
    return best * 1e6


def prompt_arm(ms):
    import ctypes
    from eetq_amd import _lib
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    out_path = os.path.join(ROOT, "profiles", "int4_prompt_direct.jsonl")
    side = torch.cuda.Stream()
    g = torch.Generator(device=dev); g.manual_seed(1)
    with open(out_path, "a") as fh:
        for K, N in SHAPES:
            nbuf = max(2, (320 << 20) // (K * N // 2))   # rotating sets: more int4 weight bytes than the 256 MB last-level cache
            sets = [(torch.randint(-128, 128, (K, N // 2), device=dev, generator=g, dtype=torch.int8),   # any byte is two nibbles
                     (torch.rand(N, device=dev, generator=g) * 0.01 + 0.005).half()) for _ in range(nbuf)]
            calls = min(2 * nbuf, 16)
            for M in ms:
                x = (torch.rand(M, K, device=dev, generator=g) - 0.5).half()
                expand = lambda i: ops.w8_a16_gemm(x, sets[i % nbuf][0], sets[i % nbuf][1], path="mfma")   # noqa: E731
                direct = lambda i: ops.w4_a16_gemm_tiled(x, sets[i % nbuf][0], sets[i % nbuf][1])          # noqa: E731
                side.wait_stream(torch.cuda.current_stream())   # x and the sets were made on the current stream
                with torch.cuda.stream(side):
                    same = torch.equal(expand(0), direct(0))   # the eager call per shape: the expansion scratch of `side` exists
                runs = {"expand": [], "direct": []}
                for _ in range(2):                             # alternating: a drift of the box hits both
                    runs["expand"].append(chain_on(side, expand, calls))
                    runs["direct"].append(chain_on(side, direct, calls))
                path, detail = ctypes.c_int(0), ctypes.c_int(0)
                _lib.check(_lib.lib().eetq_diag_auto_path(8, M, N, K, ctypes.byref(path), ctypes.byref(detail)))
                e, d = min(runs["expand"]), min(runs["direct"])
                line = json.dumps({"K": K, "N": N, "M": M, "expand_us": round(e, 2), "direct_us": round(d, 2), "direct_over_expand": round(d / e, 3),
                                   "expand_runs_us": [round(v, 2) for v in runs["expand"]], "direct_runs_us": [round(v, 2) for v in runs["direct"]],
                                   "direct_tiles": direct_plan(M, N, K, n_cu), "expand_w8_auto_path": [path.value, detail.value], "equal": bool(same), "cus": n_cu})
                print(line, flush=True)
                fh.write(line + "\n")
                fh.flush()
            del sets
            torch.cuda.empty_cache()


if "--prompt" in sys.argv:
    rest = [a for a in sys.argv[1:] if a != "--prompt"]
    prompt_arm(tuple(int(a) for a in rest[0].split(",")) if rest else (129, 256, 512, 1024, 4096))
    sys.exit(0)

for K, N in [(4096, 4096), (4096, 11008), (11008, 4096), (5120, 5120), (5120, 13824), (13824, 5120)]:
    nbuf = max(2, (640 << 20) // (K * N))
    g = torch.Generator(device=dev); g.manual_seed(1)
    s8, s4 = [], []
    for i in range(nbuf):
        w = ((torch.rand(K, N, device=dev, generator=g) * 2 - 1) / K ** 0.5).half()
        s8.append(tuple(ops.quant_weights(w, torch.int8, False)))
        s4.append(tuple(ops.quant_weights(w, torch.quint4x2, False)))
        del w
    for M in (tuple(int(a) for a in sys.argv[1].split(',')) if len(sys.argv) > 1 else (1, 4, 8, 64)):
        x = torch.rand(M, K, device=dev, generator=g).half()
        out = {}
        for name, sets in (("w8", s8), ("w4", s4)):
            def step(i):
                ops.w8_a16_gemm(x, sets[i % nbuf][0], sets[i % nbuf][1])
            try:
                out[name] = chain_us(step, 2 * nbuf)
            except Exception:  # noqa: BLE001  W4A16 prefill expands into a per-stream scratch that cannot be created during
                # capture: time an eager loop instead (host launch time included)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(100):
                    step(i)
                b.record()
                torch.cuda.synchronize()
                out[name] = a.elapsed_time(b) * 10.0
                out[name + "_eager"] = True
        wbytes8 = K * N
        print(json.dumps({"K": K, "N": N, "M": M, "w8a16_us": round(out["w8"], 2), "w4a16_us": round(out["w4"], 2), "w4_timed_eagerly": bool(out.get("w4_eager", False)),
                          "w8_GBps": round((wbytes8 + 2*M*K + 2*N + 2*M*N) / out["w8"] / 1e3),
                          "w4_GBps": round((wbytes8 / 2 + 2*M*K + 2*N + 2*M*N) / out["w4"] / 1e3)}), flush=True)
    del s8, s4; torch.cuda.empty_cache()
