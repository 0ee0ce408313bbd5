#!/usr/bin/env python
"""Benchmark of the W8A16 hot path on MI355X.  Contract: python bench.py --gpus N --steps K --warmup W
(for N > 1 launched by torch.distributed.run, one rank per GPU); rank 0 prints ONE JSON line.

Workload (BASELINE.json configs[1], the configuration the metric is quoted on): w8a16 GEMV, M=1, N=K=4096.
A "step" is one w8_a16_gemm call (one pass of the decode hot path over one batch) on the next of NBUF distinct
(weight, scale) sets -- NBUF*16 MiB >= 512 MiB, so the weights come from HBM, not the 256 MB Infinity Cache.

A plain run does only what the headline needs: set-up, W eager warm-up steps, the K timed steps, the outputs of the last
step when --dump-outputs DIR is given, the JSON line.  Everything below `value` is measured only with --full.

  value      whole-job GB/s: algorithmic bytes (K*N + 2*M*K + 2*N + 2*M*N = 16 801 792 B/step) x K x replicas / wall
             time of the timed region.  The timed region is exactly K dependent launches, captured as HIP graphs: one graph
             of K launches when K <= 2000, else a graph of 2000 launches (a whole number of passes over the weight sets)
             replayed K // 2000 times and one graph of the remainder, so the ~7 us between two graph replays is spread over
             2000 steps once K is that large.  Barrier + synchronize on both sides and the MAX over ranks.
             ms_per_step = region / K; timed_steps = K and timed_ms = the region.  Includes the ~1.5-1.9 us dependent-kernel
             boundary of every step and, spread over the K steps, the launch of the first graph: choose K from
             ms_per_step so that the region is long (K = 20: 5.5-5.7 us per step, K = 200 000: 4.43 us, the latter
             what the >= 50 ms regions of earlier rounds measured).
  --dump-outputs DIR   DIR/gemv_y.npy: the [M, N] result of the last timed step (float32 of the fp16 output).  The inputs are
             seeded, so two runs with the same arguments compute from the same weights and activations.
  roofline   dominant kernel (gemv_kernel): algorithmic bytes / kernel duration, where the duration comes from a region of its
             own, timed like the headline before K set the timed steps: ONE graph of dependent launches whose length does not
             depend on K (the smallest common multiple of K and NBUF that is >= 1000 launches) replayed until the region is at
             least --min-timed-ms long (default 50 ms), divided by the launches (the rocprofv3 trace of
             this command shows <= 0.1 us between consecutive dispatches, so this is the kernel's begin->end plus that gap:
             an upper bound, never an underestimate).  HIP start/stop event pairs per dispatch are NOT used for the figure:
             the method's own floor is ~4.2 us (an empty kernel reads 4.25 us), i.e. it cannot see a 4-5 us kernel; they are
             kept as a diagnostic and marked invalid whenever they sit within 10 % of that floor.  `rocprof` repeats the
             average of the same kernel from the committed rocprofv3 --kernel-trace --stats summary of this command
             (profiles/rNN_bench_kernel_stats.csv, written by tools/profile_bench.sh together with the commit it was taken at
             and a hash of the kernel sources, which is compared with the sources of this run).  `traffic` = HBM/fabric
             bytes per launch from the PMC passes of the same script (profiles/pmc_traffic.json, stamped the same way).
             roofline.gemm_m1024: the other half of the metric, fused dequant-GEMM at M=1024 (MFMA roofline), same method.
  cpu_baseline  the oracle's scalar C port of the same GEMV on one host core (bounded sample); beside it
             (cpu_linear_fp16) the north star's CPU torch.nn.Linear fp16 forward, best over a sweep of thread counts.
  config4    BASELINE configs[3]: the Llama-2-7B projection shapes x M in {1, 8, 64, 1024} (+ 32 / 128 / 256 at
             4096^2) through AUTO, each chain-timed like the roofline, with the path AUTO took, both roofline fractions and a
             tier-A check against the oracle (skip with --no-config4).  Reported beside the headline, never as `value`.
  config5    BASELINE configs[4] on the same box (skip with --no-config5): Llama-2-13B shapes, prompt 1024 + 50 new tokens,
             one replica per GPU, whole-job tokens/s.  Reported beside the headline, never as `value`.
  parity     (rank 0) the headline's output against the oracle, the packed weights bit for bit, and across replicas.
Multi-GPU: replicas only (model replicated, no data-path collective); rank 0 fans the activations out with one
broadcast; with --full the results are checked to be bit-identical across replicas.  scaling = "weak".
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0      # MI355X_MICROARCH.md: 8 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16/bf16 MFMA


def gemv_bytes(M, N, K):
    return K * N + 2 * M * K + 2 * N + 2 * M * N


def make_weight_sets(ops, nbuf, K, N, dev):
    """set 0 = nn.Linear default init, seed 1 (the recipe of examples/layers/test_qlinear.py); the others are
    U(+-1/sqrt(K)) drawn on the GPU.  All quantised by the HIP quantiser on the GPU."""
    sets = []
    torch.manual_seed(1)
    lin = torch.nn.Linear(K, N, bias=False, dtype=torch.float16)
    w0 = lin.weight.detach().t().contiguous()
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    bound = 1.0 / (K ** 0.5)
    for i in range(nbuf):
        if i == 0:
            w = w0.to(dev)
        else:
            w = ((torch.rand(K, N, device=dev, generator=g) * 2 - 1) * bound).half()
        processed, scales = ops.quant_weights(w, torch.int8, False)
        sets.append((processed, scales))
        del w
    return sets, w0, lin


GRAPH_MIN_LAUNCHES = 1000   # a captured graph holds at least this many launches whatever --steps is


def graph_length(nsteps, nbuf, min_launches=GRAPH_MIN_LAUNCHES):
    """Launches per captured graph: the smallest common multiple of `nsteps` (so the timed region is a whole number of
    K-step sequences) and `nbuf` (so every weight set is visited equally often) that is >= min_launches.  The length does
    NOT shrink with --steps: a 20-launch graph spreads the ~7 us between two graph replays over 20 steps (+0.34 us per
    4.6 us step, the round-3 driver line), a 1000-launch graph over 1000."""
    unit = nsteps * nbuf // math.gcd(nsteps, nbuf)
    if unit > 20000:   # odd --steps: keep whole K-step sequences, let the last pass over the sets be partial
        unit = nsteps
    return unit * max(1, -(-min_launches // unit))


def warm_side_stream(fn):
    """fn(0, 3) on a side stream before a capture: lazy initialisation happens outside the capture."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(0, 3)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    from eetq_amd import ops as _ops
    _ops.release_stream_workspace(s)   # the warm-up stream's split-K scratch region, if it took one (config4 captures 15 graphs)


def capture_graphs(fn, nsteps, nbuf, min_launches=GRAPH_MIN_LAUNCHES):
    """ONE graph of graph_length(nsteps, nbuf) dependent launches = the K-step sequence repeated, continuing the rotation
    over the weight sets (step i uses set i % nbuf), so the graph is a whole number of K-step sequences and of passes over
    the sets.  Returned as a list for timed_replays()."""
    length = graph_length(nsteps, nbuf, min_launches)
    warm_side_stream(fn)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for first in range(0, length, nsteps):
            fn(first, nsteps)
    return [g], length


HEADLINE_GRAPH_MAX = 2000   # launches per captured graph of the headline's timed region


def exact_step_graphs(fn, nsteps, rotation, max_launches=HEADLINE_GRAPH_MAX):
    """Graphs whose replays issue exactly `nsteps` dependent launches fn(i) for i = 0 .. nsteps - 1, in order: ONE graph of
    nsteps launches when nsteps <= max_launches, else a body graph of L launches (a multiple of `rotation`, the period of
    the step's buffers, so every replay continues where the last one stopped) replayed nsteps // L times and one graph of
    the remainder.  Returns [(graph, launches, replays)]."""
    warm_side_stream(fn)

    def capture(first, count):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(first, count)
        return g
    body = rotation * max(1, max_launches // rotation)
    if nsteps <= body:
        return [(capture(0, nsteps), nsteps, 1)]
    reps, rest = divmod(nsteps, body)
    plan = [(capture(0, body), body, reps)]
    if rest:
        plan.append((capture(reps * body, rest), rest, 1))
    return plan


def timed_replays(grp, graphs, nsteps, min_seconds):
    """Replays the graphs round-robin for >= min_seconds (a whole number of rounds); returns (seconds, replays)."""
    for g in graphs:  # one untimed replay each: graph upload
        g.replay()
    grp.synchronize()
    t0 = time.perf_counter()
    for g in graphs:
        g.replay()
    grp.synchronize()
    est = max((time.perf_counter() - t0) / len(graphs), 1e-6)      # seconds per replay (incl. launch latency: an upper bound)
    rounds = max(1, int(math.ceil(min_seconds / est / len(graphs))))
    if grp.world_size > 1:  # every rank must time the same amount of work
        rounds = int(grp.max_over_ranks(float(rounds)))

    def run():
        for _ in range(rounds):
            for g in graphs:
                g.replay()
    seconds = grp.timed(run)
    if seconds < min_seconds:  # the estimate included host latency: top up once
        rounds = int(math.ceil(rounds * min_seconds / seconds * 1.1))
        if grp.world_size > 1:
            rounds = int(grp.max_over_ranks(float(rounds)))
        seconds = grp.timed(run)
    return seconds, rounds * len(graphs)


def stamped_chain(grp, fn, nlaunches, min_seconds):
    """Times `nlaunches` dependent launches issued by fn(first, count), captured as ONE graph between two clock-stamp
    launches (eetq_diag_clock_stamp: 512 one-wave workgroups record XCC_ID, s_memtime = shader cycles, s_memrealtime =
    100 MHz), replayed for >= min_seconds.  Returns (us per launch, effective shader clock in MHz = median over the XCDs of
    d(memtime) / d(memrealtime) x 100 over the last replay, number of XCDs seen)."""
    from eetq_amd import _lib
    L = _lib.lib()
    dev = grp.device
    nwg = 512
    a = torch.zeros(nwg * 4, dtype=torch.int64, device=dev)
    b = torch.zeros(nwg * 4, dtype=torch.int64, device=dev)

    def body(first, count):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.eetq_diag_clock_stamp(ctypes.c_void_p(a.data_ptr()), nwg, st))
        fn(first, count)
        _lib.check(L.eetq_diag_clock_stamp(ctypes.c_void_p(b.data_ptr()), nwg, st))
    graphs, _ = capture_graphs(body, nlaunches, 1, nlaunches)
    seconds, replays = timed_replays(grp, graphs, nlaunches, min_seconds)
    sa = a.cpu().numpy().reshape(nwg, 4)
    sb = b.cpu().numpy().reshape(nwg, 4)
    mhz = []
    for xcc in sorted(set(sa[:, 0].tolist()) & set(sb[:, 0].tolist())):
        ra = sa[sa[:, 0] == xcc][0]
        rb = sb[sb[:, 0] == xcc][0]
        dt = float(rb[3] - ra[3])
        if dt > 0:
            mhz.append(float(rb[2] - ra[2]) / dt * 100.0)
    return seconds * 1e6 / (replays * nlaunches), (float(np.median(mhz)) if mhz else None), len(mhz)


def dispatch_kernel_time(run, nlaunches):
    """Mean/median/min kernel duration (seconds) of `nlaunches` launches issued by run(): every launch carries a HIP
    start/stop event pair on its dispatch packet (eetq_prof_begin/_end -> hipExtLaunchKernelGGL), i.e. the kernel's own
    begin/end timestamps -- the quantity rocprofv3 --kernel-trace reports -- on the stream the kernel is launched on."""
    from eetq_amd import _lib
    L = _lib.lib()
    _lib.check(L.eetq_prof_begin(nlaunches))
    run()
    buf = (ctypes.c_float * nlaunches)()
    cnt = ctypes.c_int(0)
    _lib.check(L.eetq_prof_end(buf, nlaunches, ctypes.byref(cnt)))
    us = np.array(buf[:cnt.value], dtype=np.float64)
    assert cnt.value == nlaunches, (cnt.value, nlaunches)
    return float(us.mean()) * 1e-6, float(np.median(us)) * 1e-6, float(us.min()) * 1e-6


def cpu_gemv_baseline(oracle, x, q, s, budget_s=10.0):
    """Oracle port (scalar C, one core) of the same GEMV; bounded sample."""
    t_end = time.perf_counter() + budget_s
    oracle.w8a16_gemm_f32acc(x, q, s)  # warm
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() < t_end or n < 3:
        oracle.w8a16_gemm_f32acc(x, q, s)
        n += 1
    dt = time.perf_counter() - t0
    return n, dt


def cpu_linear_sweep(lins, x, runs, thread_counts):
    """CPU nn.Linear fp16 forward (north-star baseline): median of `runs` calls per thread count, call i on lins[i % len]
    (one module = the same 32 MiB weight every call, i.e. served from the host's caches; many modules = rotated like the
    GPU side rotates its weight sets); returns {threads: seconds}."""
    out = {}
    keep = torch.get_num_threads()
    try:
        with torch.no_grad():
            for t in thread_counts:
                torch.set_num_threads(t)
                for i in range(2):
                    lins[i % len(lins)](x)
                ts = []
                for i in range(runs):
                    lin = lins[(i + 2) % len(lins)]
                    t0 = time.perf_counter()
                    lin(x)
                    ts.append(time.perf_counter() - t0)
                out[t] = float(np.median(ts))
    finally:
        torch.set_num_threads(keep)
    return out


def rotated_cpu_linears(lin, count):
    """`count` fp16 nn.Linear modules of lin's shape with distinct weights (count x 32 MiB at 4096^2: >= 512 MiB, larger than
    the host's last-level caches, as the GPU side's 640 MiB of weight sets is larger than the Infinity Cache)."""
    out = [lin]
    g = torch.Generator().manual_seed(7)
    for _ in range(count - 1):
        m = torch.nn.Linear(lin.in_features, lin.out_features, bias=False, dtype=torch.float16)
        with torch.no_grad():
            m.weight.copy_(((torch.rand(lin.weight.shape, generator=g) * 2 - 1) / lin.in_features ** 0.5).half())
        out.append(m)
    return out


KERNEL_SOURCES = ("eetq_amd/csrc/common.hpp", "eetq_amd/csrc/gemv_kernel.hpp", "eetq_amd/csrc/gemv.hip",
                  "eetq_amd/csrc/gemm_kernel.hpp", "eetq_amd/csrc/gemm.hip")


def kernel_source_sha16():
    """sha256 (first 16 hex digits) over the sources of the two headline kernels: profiles/ files carry the value they
    were measured at, so a stale profile is visible in the bench line."""
    import hashlib
    h = hashlib.sha256()
    for rel in KERNEL_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def load_profile_docs():
    """(pmc traffic doc, rocprof summary doc) committed under profiles/ by tools/profile_bench.sh; {} when absent."""
    docs = []
    for name in ("pmc_traffic.json", "bench_rocprof.json"):
        try:
            docs.append(json.load(open(os.path.join(ROOT, "profiles", name))))
        except Exception:
            docs.append({})
    return docs


def decode_budget(dec, model, prompt):
    """Where one decoded token's time goes (batch 1), in microseconds by kernel family:
      * `step_us`: one replay of the decoder's HIP graph, mean of 20 back-to-back replays (barrier on both sides);
      * per family: the begin -> end durations of the library's launches of ONE eager step (eetq_prof_begin/_end: start / stop
        events on the dispatch packets, the quantity rocprofv3 --kernel-trace reports), assigned by launch order -- five launches
        per decoder layer: norm + q|k|v GEMV, rotary + cache write + attention, o GEMV + residual, norm + gate|up GEMV + SiLU,
        down GEMV + residual -- with the algorithmic bytes each family streams per token;
      * `head_us`: embedding, final norm, fp16 lm_head GEMM and the argmax + token hand-over launch timed as their own graph;
      * `gaps_us` = step - (sum of the above): what lies BETWEEN the dispatches of the graph (the dependent-launch boundaries).
    The sums reproduce the step by construction; `gap_per_launch_us` says how."""
    from eetq_amd import _lib
    L = _lib.lib()
    base = model.model
    layers = len(base.layers)
    cfg = model.config
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    dev = dec.device
    if dec.graph is None or not dec._lean():
        return None
    with torch.no_grad():
        dec.generate(prompt, 8)   # the cache back at prompt + 8 rows: the 21 steps below stay inside its capacity
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        dec.graph.replay()
    torch.cuda.synchronize()
    step_us = (time.perf_counter() - t0) / 20 * 1e6
    cap = layers * 8 + 64
    _lib.check(L.eetq_prof_begin(cap))
    with torch.no_grad():
        dec._step()
    buf = (ctypes.c_float * cap)()
    cnt = ctypes.c_int(0)
    _lib.check(L.eetq_prof_end(buf, cap, ctypes.byref(cnt)))
    us = np.array(buf[:cnt.value], dtype=np.float64)
    per_layer = 5
    if cnt.value < layers * per_layer:
        return {"skipped": "expected %d library launches in an eager step, saw %d" % (layers * per_layer, cnt.value)}
    body = us[:layers * per_layer].reshape(layers, per_layer)
    rows = int(dec.s_pos.item()) + 1
    kv_bytes = 2 * cfg.num_key_value_heads * rows * (H // cfg.num_attention_heads) * 2
    fam = [("qkv_gemv", H * 3 * H), ("rope_attn_decode", kv_bytes), ("o_gemv", H * H), ("gate_up_gemv", H * 2 * I),
           ("down_gemv", I * H)]
    out = {"step_us": round(step_us, 1), "families": {}}
    total = 0.0
    for i, (name, nbytes) in enumerate(fam):
        t = float(body[:, i].sum())
        total += t
        out["families"][name] = {"us_per_token": round(t, 1), "us_per_launch": round(t / layers, 2),
                                 "TBps": round(nbytes / (t / layers) / 1e6, 2)}
    tail = float(us[layers * per_layer:].sum())   # library launches after the last layer (final norm)
    # embedding + final norm + lm_head + argmax as their own graph
    h = torch.zeros(dec.batch, 1, H, dtype=torch.float16, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        sc_out, sc_tok = torch.zeros_like(dec.out_buf), torch.zeros_like(dec.s_tok)
        sc_pos, sc_idx = torch.zeros_like(dec.s_pos), torch.zeros_like(dec.s_idx)

        def head():   # embedding, final norm, lm_head and the step's hand-over exactly as GraphDecoder._advance runs them
            e = base.embed_tokens(dec.s_tok)
            lg = model.lm_head(base.norm(h + e))[:, -1]
            import eetq_amd.ops as _ops
            _ops.greedy_handover(lg, sc_out, sc_idx, sc_tok, sc_pos)   # argmax + hand-over, one launch (a column beyond the
            #                                                             scratch buffer is skipped by the kernel)
        head()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            head()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    head_us = (time.perf_counter() - t0) / 20 * 1e6
    del g
    launches = layers * per_layer
    out["head_us"] = round(head_us, 1)
    out["library_tail_us"] = round(tail, 1)
    out["kernels_us"] = round(total, 1)
    out["gaps_us"] = round(step_us - total - head_us, 1)
    out["gap_per_launch_us"] = round((step_us - total - head_us) / launches, 2)
    out["weight_floor_us"] = round(layers * (4 * H * H + 3 * H * I) / 8e6, 1)
    out["note"] = ("step = %d layer launches (begin -> end, one eager step) + head (embedding, norm, fp16 lm_head, argmax, token "
                   "hand-over as a graph) + gaps (the remainder: dependent-launch boundaries inside the graph); weight_floor = int8 layer "
                   "weights / 8 TB/s" % launches)
    return out


def config5_leg(grp, prompt_len=1024, new_tokens=50):
    """BASELINE configs[4] on every replica: random-init Llama-2-13B shapes (no checkpoints offline), eet_accelerator with
    W8A16 everywhere, identical prompt fanned out from rank 0, greedy decode of 50 tokens through the HIP-graph decoder.
    Whole-job tokens/s = replicas x 50 / MAX over ranks of the end-to-end time (prefill + decode).  None when transformers
    is not importable."""
    try:
        import transformers
        from eetq_amd.utils import GraphDecoder, eet_accelerator
    except Exception as e:  # noqa: BLE001
        return {"skipped": "transformers / accelerator not importable: %s" % (str(e)[:80],)}
    dev = grp.device
    cfg = transformers.LlamaConfig(hidden_size=5120, intermediate_size=13824, num_hidden_layers=40, num_attention_heads=40,
                                   num_key_value_heads=40, vocab_size=32000, max_position_embeddings=4096)
    torch.manual_seed(0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device(dev):
            model = transformers.LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(old)
    eet_accelerator(model, quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)
    prompt = torch.randint(0, 32000, (4, prompt_len), generator=torch.Generator().manual_seed(1)).to(dev)
    grp.fan_out(prompt)
    batches = {}
    crcs = []
    res = None
    with torch.no_grad():
        # batch 1 is the configuration BASELINE configs[4] names; 2 and 4 mirror the reference's own published table
        # (README.md:109-113: 37.17 / 54.01 / 69.79 tokens/s on an RTX 3090)
        for B in (1, 2, 4):
            holder = {}
            dec = GraphDecoder(model, B, prompt_len + new_tokens + 8)
            # warm-up with the SAME prompt and length as the timed call, like the reference's recipe
            # (examples/models/llama_transformers_example.py:68-79: one generate with the same arguments, then the timed one):
            # a short warm-up left the first full-length prefill's one-time costs (allocator growth, first use of the M = 1024
            # kernels) inside the timed region, 6 ms of 180 (tools/decode_timeline.py)
            dec.generate(prompt[:B], new_tokens)
            torch.cuda.synchronize()

            def run():
                holder["out"] = dec.generate(prompt[:B], new_tokens)
            secs = grp.timed(run)
            # the prompt pass as generate() runs it (GraphDecoder.prefill: static cache, counters reset, causal rows only, last-position
            # logits); rounds 2-5 timed a cache-less model(prompt) here, which takes another attention path
            t_prefill = grp.timed(lambda: dec.prefill(prompt[:B]))
            c = grp.gather_checksums(holder["out"][:, prompt_len:].to(torch.int32))
            crcs.append(len(set(c)) == 1)
            batches[str(B)] = {"tokens_per_s": round(grp.world_size * B * new_tokens / secs, 2), "end_to_end_s": round(secs, 4),
                               "prefill_s": round(t_prefill, 4)}
            budget = None
            if B == 1 and grp.rank == 0:
                try:
                    budget = decode_budget(dec, model, prompt[:B])
                except Exception as e:  # noqa: BLE001  (diagnostic: never fails the bench line)
                    budget = {"skipped": str(e)[:120]}
            if B == 1:
                res = {"workload": "Llama-2-13B shapes (random init), eet_accelerator W8A16, prompt %d + %d new tokens, batch 1 "
                                   "per replica, HIP-graph greedy decode" % (prompt_len, new_tokens),
                       "tokens_per_s": batches["1"]["tokens_per_s"], "end_to_end_s": batches["1"]["end_to_end_s"],
                       "prefill_s": batches["1"]["prefill_s"], "replicas": grp.world_size, "decode_budget": budget}
            del dec
            torch.cuda.empty_cache()
    res["replicas_identical_tokens"] = all(crcs)
    res["batches"] = batches
    res["batches_note"] = ("whole-job tokens/s = replicas x batch x %d / MAX-over-ranks end-to-end time (prefill + decode); "
                           "reference README.md:109-113 (RTX 3090): 37.17 / 54.01 / 69.79 at batch 1 / 2 / 4" % new_tokens)
    del model
    torch.cuda.empty_cache()
    return res


PATH_NAMES = {0: "auto", 1: "gemv", 2: "mfma", 3: "stream", 4: "mid", 5: "splitk", 6: "tilesplit"}


def auto_path_name(bits, M, N, K):
    """What EETQ_PATH_AUTO launches for this problem (eetq_diag_auto_path: the function the launchers call, host arithmetic)."""
    from eetq_amd import _lib
    p, d = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().eetq_diag_auto_path(bits, M, N, K, ctypes.byref(p), ctypes.byref(d)))
    name = PATH_NAMES.get(p.value, str(p.value))
    if p.value == 6:
        name = "tilesplit/S=%d" % d.value if d.value > 1 else "tile"
    if p.value == 2:
        name = "tile"
    if p.value == 5 and d.value > 0:
        name = "splitk/rows=%d" % d.value
    if p.value == 3:
        f, t, w = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        if M <= 16 and _lib.lib().eetq_diag_stream_plan(bits, M, N, K, 0, ctypes.byref(f), ctypes.byref(t), ctypes.byref(w)) == 0:
            name = "stream/%s,%d,%d" % (("regs", "block", "ring")[f.value], t.value, w.value)
    return name


CONFIG4_SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))          # (K, N): q/k/v/o, gate/up, down of Llama-2-7B
CONFIG4_MS = {(4096, 4096): (1, 8, 32, 64, 128, 256, 1024)}           # M in {1, 8, 64, 1024}; 4096^2 also 32 / 128 / 256
CONFIG4_DEFAULT_MS = (1, 8, 64, 1024)


def config4_leg(grp, ops, oracle, sets4096, min_s=0.03):
    """BASELINE configs[3] (SURVEY 8(d) "Config 4 sweep"): the Llama-2-7B projection shapes x M in {1, 8, 64, 1024}, plus
    M in {32, 128, 256} at 4096^2, through EETQ_PATH_AUTO -- every point timed like the headline (ONE HIP graph of >= 1000
    dependent launches -- >= 200 at M = 1024 -- over rotating weight sets larger than the Infinity Cache, replayed twice for >= 15 ms: the better region),
    with the path AUTO took, both roofline fractions and a tier-A check of the point's own output against the oracle on the
    last 256 columns (the oracle quantises those columns of the fp16 weight itself, so the GPU quantiser is in the loop).
    Labelled extra, never `value`.  Every rank runs it (the timed regions hold barriers); rank 0 reports."""
    dev = grp.device
    t_start = time.perf_counter()
    points = []
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    for (K, N) in CONFIG4_SHAPES:
        bound = 1.0 / (K ** 0.5)
        w_first = ((torch.rand(K, N, device=dev, generator=g) * 2 - 1) * bound).half()
        if (K, N) == (4096, 4096):
            sets = [ops.quant_weights(w_first, torch.int8, False)] + list(sets4096[1:])
        else:   # 16 x 43 MiB = 688 MiB > Infinity Cache
            sets = [ops.quant_weights(w_first, torch.int8, False)]
            for _ in range(15):
                sets.append(ops.quant_weights(((torch.rand(K, N, device=dev, generator=g) * 2 - 1) * bound).half(), torch.int8, False))
        nbuf = len(sets)
        cols = slice(N - 256, N)
        w_cols = w_first[:, cols].cpu().numpy() if oracle is not None else None
        del w_first
        q_cols = s_cols = None
        if oracle is not None:
            q_cols, s_cols = oracle.quantize(np.ascontiguousarray(w_cols))
        for M in CONFIG4_MS.get((K, N), CONFIG4_DEFAULT_MS):
            torch.manual_seed(100 + M)
            x = torch.rand(M, K, dtype=torch.float16).to(dev)
            grp.fan_out(x)
            outs = [torch.empty(M, N, dtype=torch.float16, device=dev) for _ in range(2)]

            def steps(first, count, x=x, outs=outs, sets=sets, nbuf=nbuf, M=M, N=N, K=K):
                for i in range(first, first + count):
                    w, sc = sets[i % nbuf]
                    ops.w8_a16_gemm_(x, w, sc, outs[i % 2], M, N, K)
            steps(0, 2 * nbuf if M < 1024 else nbuf)     # warm-up: kernel selection, scratch, clocks
            grp.synchronize()
            launches = 1000 if M < 1024 else 200
            launches = -(-launches // nbuf) * nbuf       # whole passes over the weight sets
            graphs, glen = capture_graphs(steps, launches, nbuf, launches)
            us, replays = None, 0
            for _ in range(2):   # the better of two timed regions: one stalled replay (seen once: 10.1 -> 17.0 us) must not stand
                secs, n = timed_replays(grp, graphs, launches, min_s / 2)
                us = secs * 1e6 / (n * glen) if us is None else min(us, secs * 1e6 / (n * glen))
                replays += n
            del graphs
            pt = {"K": K, "N": N, "M": M, "us": round(us, 3), "path": auto_path_name(8, M, N, K),
                  "hbm_frac": round(gemv_bytes(M, N, K) / (us * 1e-6) / 1e9 / HBM_PEAK_GBPS, 4),
                  "mfma_frac": round(2.0 * M * N * K / (us * 1e-6) / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                  "GBps": round(gemv_bytes(M, N, K) / (us * 1e-6) / 1e9, 1),
                  "TFLOPS": round(2.0 * M * N * K / (us * 1e-6) / 1e12, 2), "launches_timed": replays * glen}
            if oracle is not None:
                rows = list(range(min(M, 8))) + list(range(max(M - 8, 8), M))          # first and last rows of the batch
                ops.w8_a16_gemm_(x, sets[0][0], sets[0][1], outs[0], M, N, K)
                got = outs[0][rows][:, cols].float().cpu().numpy()
                ref = oracle.w8a16_gemm(x[rows].cpu().numpy(), q_cols, s_cols).astype(np.float32)
                pt["tier_a_ok"] = bool(np.all(np.abs(got - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)))
            points.append(pt)
        del sets
        torch.cuda.empty_cache()
    return {"what": "BASELINE configs[3] / SURVEY 8(d) config-4 sweep through EETQ_PATH_AUTO: (K, N) in {(4096, 4096), (4096, 11008), "
                    "(11008, 4096)} x M in {1, 8, 64, 1024} (+ M in {32, 128, 256} at 4096^2); per point one HIP graph of >= 1000 "
                    "dependent launches (>= 200 at M = 1024) over rotating weight sets (40 x 16 MiB / 16 x 43 MiB), replayed twice for >= 15 ms, the better region counts; "
                    "hbm_frac = (K*N + 2*M*K + 2*N + 2*M*N) B / us / 8 TB/s, mfma_frac = 2*M*N*K / us / 2.5 PF; tier_a_ok = this "
                    "point's output vs the oracle on the last 256 columns, first and last 8 rows",
            "points": points, "all_tier_a_ok": all(p.get("tier_a_ok", True) for p in points),
            "seconds": round(time.perf_counter() - t_start, 2)}


def full_legs(args, grp, ops, sets, x, outs, gemv_steps, w0_cpu, lin_cpu):
    """--full: everything the line carries beside the headline -- parity against the oracle, the roofline of the GEMV (its own
    region, see the module docstring) with the event-pair diagnostic and the grouped form, the M = 1024 GEMM with its power
    check, the CPU baselines, the quantiser, config4 and config5.  Returns the line's keys for them."""
    from eetq_amd import _lib
    dev = grp.device
    M, K = x.shape
    N = outs[0].shape[1]
    steps, nbuf = args.steps, args.nbuf
    min_s = args.min_timed_ms * 1e-3


    # ---- parity of this run (rank 0 checks against the oracle; all ranks must agree bit for bit) ----
    parity = {}
    y0 = torch.empty(M, N, dtype=torch.float16, device=dev)
    ops.w8_a16_gemm_(x, sets[0][0], sets[0][1], y0, M, N, K)
    torch.cuda.synchronize()
    crcs = grp.gather_checksums(y0)
    parity["replicas_bit_identical"] = len(set(crcs)) == 1
    oracle = None
    if grp.rank == 0:
        import oracle as _oracle
        oracle = _oracle
        q, s = oracle.quantize(w0_cpu.numpy())
        ref = oracle.w8a16_gemm(x.cpu().numpy(), q, s).astype(np.float32)
        got = y0.cpu().numpy().astype(np.float32)
        parity["tier_a_max_abs_err_vs_oracle"] = float(np.abs(got - ref).max())
        parity["tier_a_ok"] = bool(np.all(np.abs(got - ref) <= 1e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)))
        with torch.no_grad():
            y_lin = lin_cpu(x.cpu()).numpy().astype(np.float32)
        parity["tier_b_max_abs_err_vs_cpu_linear_fp16"] = float(np.abs(got - y_lin).max())
        parity["packed_bit_exact"] = bool(np.array_equal(sets[0][0].cpu().numpy(), oracle.gfx950_pack(q)))

    # ---- the roofline's own region: K-step graphs of >= 1000 launches replayed for >= min_timed_ms ----
    graphs, graph_len = capture_graphs(gemv_steps, steps, nbuf)
    seconds, replays = timed_replays(grp, graphs, steps, min_s)
    timed_steps = replays * graph_len
    step_bytes = gemv_bytes(M, N, K)
    del graphs

    # ---- roofline of the dominant kernel: the graph-replayed dependent chain / K is the kernel duration (see docstring) ----
    step_s = seconds / timed_steps
    achieved = step_bytes / step_s / 1e9
    src_sha = kernel_source_sha16()
    traffic_doc, rocprof_doc = load_profile_docs()

    def rocprof_ref(key, work, peak_scale):
        r = rocprof_doc.get(key)
        if not r:
            return None
        out = {"avg_us": r.get("avg_us"), "median_us": r.get("median_us"), "calls": r.get("calls"), "min_us": r.get("min_us"),
               "frac": round(work / (r["avg_us"] * 1e-6) / peak_scale, 4) if r.get("avg_us") else None,
               # the SAME profiled process's own chain step (bench.py's timed region while rocprofv3 was attached) and the
               # un-profiled chain step of the same script run: the attached tool stretches every dispatch, so the profiled
               # average is explained by chain_us_same_process (>= avg_us: a chain step is the kernel plus the inter-dispatch
               # gap), never by the un-profiled step of another process; profiler_offset_us = the difference of the two chains
               "chain_us_same_process": r.get("chain_us_same_process"),
               "chain_us_unprofiled_same_run": r.get("chain_us_unprofiled"),
               "profiler_offset_us": r.get("profiler_offset_us"),
               "file": rocprof_doc.get("file"), "head": rocprof_doc.get("head"),
               "kernel_sources_unchanged_since": rocprof_doc.get("kernel_src_sha16") == src_sha}
        # the traced MEDIAN is the figure held against the chain step (the mean carries the cold first launches and the warm-up at
        # unsettled clocks); both flags are printed
        if r.get("avg_us") and r.get("chain_us_same_process"):
            out["avg_le_chain_same_process"] = bool(r["avg_us"] <= r["chain_us_same_process"] * 1.005)
            if r.get("median_us"):
                out["median_le_chain_same_process"] = bool(r["median_us"] <= r["chain_us_same_process"] * 1.005)
            ok = out.get("median_le_chain_same_process", out["avg_le_chain_same_process"])
            if not ok:
                print("warning: profiles/%s: the traced %s dispatches (median %s / mean %.3f us) exceed the profiled process's own "
                      "chain step (%.3f us)" % (rocprof_doc.get("file"), key, r.get("median_us"), r["avg_us"],
                                                r["chain_us_same_process"]), file=sys.stderr)
        return out

    # diagnostic only: HIP event pairs on each dispatch packet, with the method's own floor (empty kernel, same geometry)
    n_ev = max(nbuf, (min(max(steps, 400), 2000) // nbuf) * nbuf)
    gemv_steps(0, nbuf)
    torch.cuda.synchronize()
    k_mean, k_med, k_min = dispatch_kernel_time(lambda: gemv_steps(0, n_ev), n_ev)
    sink = torch.zeros(16, dtype=torch.int32, device=dev)
    stream_ptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib()

    def empty():
        for i in range(n_ev):
            _lib.check(L.eetq_diag_empty(ctypes.c_void_p(sink.data_ptr()), N // 16, 1024, stream_ptr))
    empty()
    torch.cuda.synchronize()
    e_mean, e_med, e_min = dispatch_kernel_time(empty, n_ev)
    ev_valid = k_mean > 1.10 * e_mean
    roofline = {"kernel": "gemv_kernel<M=1,16 waves x 4 tiles,exact,xreg>", "bound": "hbm", "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 4),
                "kernel_us": round(step_s * 1e6, 3), "launches_timed": timed_steps,
                "method": "dependent launches replayed as HIP graphs / launches (a graph of >= 1000 launches replayed for >= "
                          "--min-timed-ms): the kernel's begin->end plus the <= 0.1 us inter-dispatch gap; NOT event pairs",
                "rocprof": rocprof_ref("gemv", step_bytes, HBM_PEAK_GBPS * 1e9),
                "traffic": traffic_doc.get("gemv_hbm_bytes_per_launch"),
                "traffic_source": {"file": "profiles/pmc_traffic.json", "how": traffic_doc.get("source"),
                                   "head": traffic_doc.get("head"),
                                   "kernel_sources_unchanged_since": traffic_doc.get("kernel_src_sha16") == src_sha},
                "algorithmic_bytes_per_launch": step_bytes, "kernel_src_sha16": src_sha,
                "event_pairs_diagnostic": {
                    "kernel_us_mean": round(k_mean * 1e6, 3) if ev_valid else None,
                    "raw_us_mean": round(k_mean * 1e6, 3), "method_floor_us": round(e_mean * 1e6, 3), "valid": bool(ev_valid),
                    "note": "start/stop events on each dispatch packet; readings within 10 % of the empty-kernel floor are "
                            "the method, not the kernel, and are withheld"}}

    # ---- labelled extra (never `value`): the same 16 MiB problems as INDEPENDENT work, 8 per dispatch ----
    # eetq_w8a16_gemv_grouped: one grid over the tile rows of 8 problems, so launch ramp / first-byte latency / tail are paid
    # once per 128 MiB instead of once per 16 MiB.  Same kernel body as the headline, bit-identical outputs.
    grouped = None
    if hasattr(ops, "w8_a16_gemv_grouped"):
        G = 8
        per_pass = nbuf // G

        def grouped_steps(first, count):
            for gi in range(first, first + count):
                idx = [(gi * G + j) % nbuf for j in range(G)]
                ops.w8_a16_gemv_grouped([x] * G, [sets[i][0] for i in idx], [sets[i][1] for i in idx])
        if per_pass >= 1 and nbuf % G == 0:
            chk = ops.w8_a16_gemv_grouped([x] * G, [sets[i][0] for i in range(G)], [sets[i][1] for i in range(G)])
            singles = [ops.w8_a16_gemm(x, sets[i][0], sets[i][1]) for i in range(G)]
            same = all(torch.equal(chk[i], singles[i]) for i in range(G))
            again = ops.w8_a16_gemv_grouped([x] * G, [sets[i][0] for i in range(G)], [sets[i][1] for i in range(G)])
            tier_a = all(bool(((chk[i].float() - singles[i].float()).abs()
                               <= 1e-3 * singles[i].float().abs().max() + 2e-3 * singles[i].float().abs()).all()) for i in range(G))
            grouped_steps(0, per_pass)
            torch.cuda.synchronize()
            gg, gg_len = capture_graphs(grouped_steps, 5 * per_pass, per_pass, 200)
            gs, gr = timed_replays(grp, gg, 5 * per_pass, min_s)
            n_prob = gr * gg_len * G
            us = gs * 1e6 / n_prob
            grouped = {"what": "eetq_w8a16_gemv_grouped: %d independent M=1, N=K=4096 problems per dispatch (graph-replayed, rotating "
                               "over the same %d weight sets); NOT the headline configuration" % (G, nbuf),
                       "problems_per_dispatch": G, "us_per_problem": round(us, 3),
                       "gbps": round(step_bytes / us / 1e3, 1), "frac_of_peak": round(step_bytes / us / 1e3 / HBM_PEAK_GBPS, 4),
                       "problems_timed": n_prob, "tier_a_vs_single_launches": bool(tier_a),
                       "bit_identical_call_to_call": all(torch.equal(chk[i], again[i]) for i in range(G)),
                       "bit_identical_to_single_launches": bool(same),
                       "note": "a dispatch with more than two tile rows per CU runs the 8-wave body (another summation order than "
                               "the 16-wave straight-line body of a separate 4096 x 4096 launch): tier A against it, not the same bits"}
            del gg
    roofline["grouped_gemv"] = grouped

    # ---- the other half of the metric: fused dequant-GEMM, M = 1024 ----
    Mg = 1024
    torch.manual_seed(2)
    xg = torch.rand(Mg, K, dtype=torch.float16).to(dev)
    yg = [torch.empty(Mg, N, dtype=torch.float16, device=dev) for _ in range(2)]

    def gemm_steps(first, count):
        for i in range(first, first + count):
            w, s = sets[i % nbuf]
            ops.w8_a16_gemm_(xg, w, s, yg[i % 2], Mg, N, K)

    gemm_steps(0, 60)  # warm-up: lets the clocks settle under MFMA load
    torch.cuda.synchronize()
    ggraphs, ggraph_len = capture_graphs(gemm_steps, args.gemm_steps, nbuf, 400)
    gsec, greplays = timed_replays(grp, ggraphs, args.gemm_steps, min_s)
    gtimed = greplays * ggraph_len
    flops = 2.0 * Mg * N * K
    g_step = gsec / gtimed
    gemm_roofline = {"kernel": "gemm_tile_kernel", "bound": "mfma", "achieved": round(flops / g_step / 1e12, 2),
                     "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(flops / g_step / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                     "kernel_us": round(g_step * 1e6, 2), "method": "graph-replayed dependent launches / launches",
                     "rocprof": rocprof_ref("gemm_m1024", flops, MFMA_F16_PEAK_TFLOPS * 1e12),
                     "traffic": traffic_doc.get("gemm_m1024_hbm_bytes_per_launch"),
                     "algorithmic_flops_per_launch": flops, "launches_timed": gtimed,
                     "whole_job_tflops": round(grp.world_size * gtimed * flops / gsec / 1e12, 2),
                     "ms_per_step": round(gsec * 1e3 / gtimed, 5), "timed_steps": gtimed}
    # Evidence for "power-bound" in the driver-run line (rank 0; labelled extras, never `value`): the same kernel and launch
    # sequence (a) as above, (b) on all-zero operands (q = 0, x = 0: nothing toggles), (c) on N(0, 0.02) weights (the shape of
    # trained weights; the BASELINE recipe's U(+-1/sqrt(K)) quantises to UNIFORM int8, the worst case for switching energy),
    # each between two device clock stamps: us per launch and the shader clock the chip held.  Every rank runs it (the timed
    # regions hold barriers); rank 0's figures are reported.
    if not args.no_power_check:
        nl = max(100, min(args.gemm_steps, 400))
        zeros_w = torch.full((K, N), -128, dtype=torch.int8, device=dev)     # processed byte 0x80 = q 0
        zeros_s = torch.ones(N, dtype=torch.float16, device=dev)
        zeros_x = torch.zeros(Mg, K, dtype=torch.float16, device=dev)
        gg3 = torch.Generator(device=dev)
        gg3.manual_seed(5)
        gsets = [ops.quant_weights((torch.randn(K, N, device=dev, generator=gg3) * 0.02).half(), torch.int8, False)
                 for _ in range(8)]

        def zero_steps(first, count):
            for i in range(first, first + count):
                ops.w8_a16_gemm_(zeros_x, zeros_w, zeros_s, yg[i % 2], Mg, N, K)

        def gauss_steps(first, count):
            for i in range(first, first + count):
                w, s = gsets[i % len(gsets)]
                ops.w8_a16_gemm_(xg, w, s, yg[i % 2], Mg, N, K)
        diag = {}
        for name, fn in (("uniform_int8_weights", gemm_steps), ("zero_operands", zero_steps),
                         ("gaussian_weights_0p02", gauss_steps)):
            fn(0, 40)
            torch.cuda.synchronize()
            us, mhz, nx = stamped_chain(grp, fn, nl, min_s)
            diag[name] = {"us": round(us, 2), "frac": round(flops / (us * 1e-6) / 1e12 / MFMA_F16_PEAK_TFLOPS, 4),
                          "effective_clock_mhz": round(mhz) if mhz else None, "xcds": nx}
        diag["what"] = ("gemm_tile_kernel M=1024, N=K=4096, %d dependent launches per graph between two clock-stamp launches "
                        "(s_memtime / s_memrealtime per XCD): `uniform_int8_weights` is the BASELINE recipe as timed above, "
                        "`zero_operands` the same instruction stream with nothing toggling, `gaussian_weights_0p02` weights "
                        "~ N(0, 0.02) (bell-shaped int8)" % nl)
        gemm_roofline["power_check"] = diag
        # the launch in SHADER CYCLES: step x the clock the chip held under this very operand set.  Cycles per launch is what the
        # code sets (58 - 61 k since round 2, whatever the box); the clock is what the box's power budget sets -- a change in
        # ms_per_step with unchanged cycles is the box, with changed cycles the code.
        mhz = diag["uniform_int8_weights"]["effective_clock_mhz"]
        if mhz:
            gemm_roofline["cycles_per_launch"] = round(diag["uniform_int8_weights"]["us"] * mhz)
            gemm_roofline["cycles_per_launch_zero_operands"] = (
                round(diag["zero_operands"]["us"] * diag["zero_operands"]["effective_clock_mhz"])
                if diag["zero_operands"]["effective_clock_mhz"] else None)
        del gsets, zeros_w, zeros_x
    roofline["gemm_m1024"] = gemm_roofline
    gemm = {"metric": "dequant-GEMM TFLOPS @ M=1024, N=K=4096", "value": gemm_roofline["whole_job_tflops"],
            "unit": "TFLOP/s", "steps": args.gemm_steps, "timed_steps": gtimed,
            "ms_per_step": gemm_roofline["ms_per_step"], "cycles_per_launch": gemm_roofline.get("cycles_per_launch"),
            "roofline": gemm_roofline}

    # ---- CPU baselines (rank 0, N = 1 only; bounded) ----
    cpu_baseline = None
    cpu_linear = None
    if grp.rank == 0 and grp.world_size == 1 and not args.no_cpu_baseline:
        q, s = oracle.quantize(w0_cpu.numpy())
        n_it, dt = cpu_gemv_baseline(oracle, x.cpu().numpy(), q, s, args.cpu_budget)
        cpu_baseline = {"value": round(n_it * step_bytes / dt / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "port",
                        "sample": "%d calls of oracle_w8a16_gemm_f32acc (scalar C restatement) at M=1, N=K=4096 in %.1f s"
                                  % (n_it, dt), "ms_per_call": round(dt / n_it * 1e3, 3)}
        ncpu = os.cpu_count() or 1
        counts = sorted(set(t for t in (8, 16, 32, 64, 128, 256, ncpu) if t <= ncpu))
        s1 = cpu_linear_sweep([lin_cpu], x.cpu(), 7, counts)
        s1024 = cpu_linear_sweep([lin_cpu], xg.cpu(), 3, counts)
        b1 = min(s1, key=s1.get)
        b1024 = min(s1024, key=s1024.get)
        # the same M = 1 call on weights rotated through 17 x 32 MiB (544 MiB), at the best thread counts of the hot sweep
        rot = rotated_cpu_linears(lin_cpu, 17)
        near = sorted(set(t for t in (b1 // 2, b1, b1 * 2) if 1 <= t <= ncpu))
        r1 = cpu_linear_sweep(rot, x.cpu(), 34, near)
        br = min(r1, key=r1.get)
        del rot
        cpu_linear = {"what": "torch.nn.Linear(4096, 4096).half() forward on host CPU (north-star baseline), best over a "
                              "sweep of torch thread counts.  m1_ms re-reads ONE 32 MiB weight (host-cache resident); "
                              "m1_rotated_ms rotates 17 distinct weights (544 MiB) like the GPU side rotates its 640 MiB",
                      "host_cores": ncpu, "m1_ms": round(s1[b1] * 1e3, 3), "m1_threads": b1,
                      "m1_gbps_fp16_weights": round(2.0 * K * N / s1[b1] / 1e9, 2),
                      "m1_rotated_ms": round(r1[br] * 1e3, 3), "m1_rotated_threads": br,
                      "m1_rotated_gbps_fp16_weights": round(2.0 * K * N / r1[br] / 1e9, 2),
                      "m1024_ms": round(s1024[b1024] * 1e3, 3), "m1024_threads": b1024,
                      "m1024_gflops": round(flops / s1024[b1024] / 1e9, 1),
                      "sweep_m1_ms": {str(t): round(v * 1e3, 2) for t, v in s1.items()},
                      "sweep_m1_rotated_ms": {str(t): round(v * 1e3, 2) for t, v in r1.items()},
                      "sweep_m1024_ms": {str(t): round(v * 1e3, 2) for t, v in s1024.items()}}

    # ---- the quantiser (model-load work, reported beside the headline, never as `value`) ----
    quantizer = None
    if grp.rank == 0:
        g2 = torch.Generator(device=dev)
        g2.manual_seed(3)
        srcs = [((torch.rand(K, N, device=dev, generator=g2) * 2 - 1) / K ** 0.5).half() for _ in range(10)]   # 320 MiB rotated
        for _ in range(3):
            ops.quant_weights(srcs[0], torch.int8, False)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(50):
            ops.quant_weights(srcs[i % 10], torch.int8, False)
        e1.record()
        torch.cuda.synchronize()
        q_us = e0.elapsed_time(e1) * 1e3 / 50
        quantizer = {"what": "quant_weights(fp16 [4096, 4096], int8) -> native layout + scales, per call, eager loop over 10 rotating "
                             "inputs (two launches: column maxima, quantise + pack); bit-exact vs the oracle in the parity block",
                     "us_per_call": round(q_us, 1), "moved_GBps": round((K * N * 2 * 2 + K * N) / q_us / 1e3)}
        del srcs

    # ---- BASELINE configs[3]: the 7B-shape sweep through AUTO (reported beside the headline, never as `value`) ----
    config4 = None
    if not args.no_config4:
        config4 = config4_leg(grp, ops, oracle, sets)

    # ---- BASELINE configs[4]: the whole decode path on the same box (reported beside the headline, never as `value`) ----
    config5 = None
    if not args.no_config5:
        config5 = config5_leg(grp)   # (the 640 MiB of weight sets stay resident; 13 GB more is no issue on 288 GB)

    return {"roofline": roofline, "secondary": gemm, "cpu_baseline": cpu_baseline, "cpu_linear_fp16": cpu_linear,
            "parity": parity, "quantizer": quantizer, "config4": config4, "config5": config5}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000, help="timed steps (GEMV launches) of the headline")
    ap.add_argument("--warmup", type=int, default=200, help="eager steps before the timed ones")
    ap.add_argument("--nbuf", type=int, default=40, help="distinct weight sets rotated per step (x16 MiB)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the output of the last timed step as DIR/gemv_y.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beside the headline too: parity against the oracle, roofline, grouped "
                         "GEMV, the M = 1024 GEMM and its power check, CPU baselines, quantiser, config4, config5")
    ap.add_argument("--min-timed-ms", type=float, default=50.0, help="--full: minimum length of every timed region")
    ap.add_argument("--gemm-steps", type=int, default=200)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-config5", action="store_true",
                    help="skip the BASELINE configs[4] leg (Llama-2-13B shapes, prompt 1024 + 50 new tokens, one replica per GPU)")
    ap.add_argument("--no-config4", action="store_true",
                    help="skip the BASELINE configs[3] sweep (7B projection shapes x M in {1, 8, 64, 1024}, + 32 / 128 / 256 at 4096^2)")
    ap.add_argument("--no-power-check", action="store_true",
                    help="skip the zero-operand / Gaussian-weight GEMM chains (tools/profile_bench.sh: the rocprofv3 average of "
                         "gemm_tile_kernel must cover the BASELINE operands only)")
    ap.add_argument("--cpu-budget", type=float, default=10.0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    from eetq_amd import ops
    from eetq_amd.utils.replicas import ReplicaGroup

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the W8A16 path has no CPU implementation)")
    grp = ReplicaGroup()
    if grp.world_size != args.gpus and grp.rank == 0:
        print("warning: --gpus %d but WORLD_SIZE=%d" % (args.gpus, grp.world_size), file=sys.stderr)
    dev = grp.device
    M, N, K = 1, 4096, 4096
    steps, warmup, nbuf = args.steps, args.warmup, args.nbuf

    sets, w0_cpu, lin_cpu = make_weight_sets(ops, nbuf, K, N, dev)
    # identical activations on every replica: rank 0 draws them, RCCL broadcast fans them out
    torch.manual_seed(1)
    x = torch.rand(M, K, dtype=torch.float16).to(dev)
    grp.fan_out(x)
    outs = [torch.empty(M, N, dtype=torch.float16, device=dev) for _ in range(8)]

    def gemv_steps(first, count):
        for i in range(first, first + count):
            w, s = sets[i % nbuf]
            ops.w8_a16_gemm_(x, w, s, outs[i % len(outs)], M, N, K)

    # ---- timed region: W warm-up steps, then exactly K steps (step i: weight set i % nbuf, output outs[i % 8]) ----
    gemv_steps(0, warmup)
    torch.cuda.synchronize()
    plan = exact_step_graphs(gemv_steps, steps, nbuf * len(outs) // math.gcd(nbuf, len(outs)))
    for g, _, _ in plan:  # one untimed replay each: graph upload
        g.replay()
    grp.synchronize()

    def run():
        for g, _, reps in plan:
            for _ in range(reps):
                g.replay()
    seconds = grp.timed(run)
    value = grp.world_size * steps * gemv_bytes(M, N, K) / seconds / 1e9
    if args.dump_outputs and grp.rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        y = outs[(steps - 1) % len(outs)]
        np.save(os.path.join(args.dump_outputs, "gemv_y.npy"), y.float().cpu().numpy())
    launch = " + ".join("%d x %d" % (reps, n) for _, n, reps in plan)
    graph_launches = plan[0][1]
    del plan

    extras = full_legs(args, grp, ops, sets, x, outs, gemv_steps, w0_cpu, lin_cpu) if args.full else {}

    if grp.rank == 0:
        line = {
            "metric": "w8a16 GEMV GB/s @ M=1 and dequant-GEMM TFLOPS @ M=1024, N=K=4096",
            "value": round(value, 1), "unit": "GB/s", "n_gpus": grp.world_size, "steps": steps, "warmup": warmup,
            "ms_per_step": round(seconds * 1e3 / steps, 6), "timed_steps": steps,
            "timed_ms": round(seconds * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": "w8a16 GEMV M=1, N=K=4096 (BASELINE configs[1]); %d distinct weight sets rotated (%d MiB)"
                                   % (nbuf, nbuf * K * N // (1 << 20)), "M": M, "N": N, "K": K,
                       "parallelism": "replicas x%d (no data-path collective)" % grp.world_size,
                       "fan_out_backend": grp.backend_note or (grp.backend if grp.world_size > 1 else "none (one replica)"),
                       "launch": "the %d timed steps as HIP graphs of dependent launches, replays x launches: %s (%.1f ms)"
                                 % (steps, launch, seconds * 1e3),
                       "graph_launches": graph_launches,
                       "timed_steps": steps, "timed_ms": round(seconds * 1e3, 3)},
        }
        line.update(extras)
        print(json.dumps(line))
    grp.close()


if __name__ == "__main__":
    main()
