"""Time one W8A16 mixture-of-experts layer (ops.w8_a16_moe) on synthetic routing; one JSON line per (shape, T, routing).

Columns: us per layer (median of --iters launches after --warmup), int8 bytes of the active experts / us, transformers' eager fp16
experts forward (MixtralExperts) on the same routing, and a Python loop of per-expert w8_a16_gemm calls (gather, gate|up with
silu_glu8, down, weighted index_add).  Weights are random (int8 stacks, small fp16 scales): the time depends on shapes only.

    python tools/moe_bench.py --out profiles/r07_moe_bench.jsonl

--backward times the training path instead, at --tokens (default 16,64,512,4096), uniform routing: the no-grad
forward (w8_a16_moe), the trainable forward (w8_a16_moe_train), the backward (w8_a16_moe_backward, both gradients) and each of
its five launches on its own, the two grouped input-gradient GEMMs against a Python loop of per-expert w8_a16_gemm_t calls after
a host read-back of the expert counts, and transformers' eager fp16 experts forward + backward (frozen fp16 stacks).  Memory:
the trainable forward's saved tensors and the backward's peak above what was allocated before it.

    python tools/moe_bench.py --backward --out profiles/r08_moe_backward_bench.jsonl

--backward --bits 4 times the int4 training path at the same shapes and token counts: the no-grad forward
(w4_a16_moe), the trainable forward (w4_a16_moe_train), the backward (w4_a16_moe_backward, both gradients) with its five launches
one at a time and its saved / peak bytes -- and, in the same process and interleaved call by call, w8_a16_moe_backward and
eetq_w8a16_moe_gemm_t on the same integers held as int8 stacks (eetq_expand_i4_to_i8, done once outside the timing), given the
same saved tensors.  Every timing is [median, min, max] us.

    python tools/moe_bench.py --backward --bits 4 --out profiles/r16_moe_int4_backward_bench.jsonl

Prompts: --tokens 64,512,4096 times the device-side prompt path; --host-path adds the column `us_host_path`, the
same layer on the former host path (one read-back of the expert counts, per-expert AUTO GEMMs), measured in a child process of its
own that sets EETQ_AMD_TUNING=1 EETQ_AMD_MOE_HOST=1 (the switch is read once per process); --no-baselines skips the fp16 eager
forward and the Python loop.

    python tools/moe_bench.py --tokens 64,512,4096 --host-path --out profiles/r09_moe_prompt_bench.jsonl

--seam sweeps the seam between the two grouped kernels: at mean rows per expert S / E = 1 .. 64 (T = rows * E / k, uniform and
skewed routing) the layer's two projections (gate|up with the gated write-out, gathered; down on the sorted rows) on
eetq_w8a16_moe_gemm and on eetq_w8a16_moe_gemm_tiled, us per pair of launches.

    python tools/moe_bench.py --seam --out profiles/r09_moe_seam.jsonl

--bits 4 times the W4A16 layer (ops.w4_a16_moe on int4 stacks; no fp16 / loop baselines) and, with --seam, its
two routes per pair of projections: eetq_w4a16_moe_gemm on the int4 tiles against eetq_expand_i4_to_i8 + eetq_w8a16_moe_gemm_tiled.
--plan-sweep times eetq_w4a16_moe_gemm's instantiations (waves x stages in flight) on every projection at T = 1, 4, 16, one
child process per plan (EETQ_AMD_TUNING=1 EETQ_AMD_MOE_I4_PLAN=<waves>x<depth>, read once per process).

    python tools/moe_bench.py --bits 4 --no-baselines --tokens 1,4,16,64,512,4096 --out profiles/r10_moe_int4_bench.jsonl
    python tools/moe_bench.py --bits 4 --seam --out profiles/r10_moe_int4_seam.jsonl      (--seam-rows: 16,32,64,128,256 by default)
    python tools/moe_bench.py --plan-sweep --out profiles/r10_moe_int4_plans.jsonl
(profiles/r10_moe_int4_plans.jsonl also holds 8x1, 4x2, 6x1 and 3x2: instantiations that lost or tied in that sweep and were
deleted after it; the sweep now covers the ones that are left.)

--path direct (with --bits 4) runs the layer table on ops.w4_a16_moe(path="direct") -- the grouped tiled kernel on the
int4 tiles -- where both projections take it (T > 16; the record's `path` says what ran), and adds to --seam a third route per pair
of projections, eetq_w4a16_moe_gemm_tiled at the launcher's tile shape (us_direct, with min and max), next to the other two.

    python tools/moe_bench.py --bits 4 --seam --path direct --out <file>.jsonl
    python tools/moe_bench.py --bits 4 --path direct --tokens 64,512,4096 --out <file>.jsonl

--block --shapes deepseek-v3 --tokens 1,4,16,64 is the same comparison under the sigmoid, bias-corrected, group-limited
rule at DeepSeek-V3's sizes (H 7168, I 2048, E 256, k 8, 8 groups, 4 kept): DeepseekV3TopkRouter's forward op for op followed by
w8_a16_moe / w4_a16_moe against ops.w8_a16_moe_block_sigmoid / w4_a16_moe_block_sigmoid, and the formula against ops.moe_router_sigmoid.

--block times the whole sparse block at --tokens (default 1,4,16,64,512), int8 or int4 experts (--bits): (a) the
sequence before the device router -- the transformers router formula in torch (F.linear, softmax(float), topk, sum, div, .to) followed
by w8_a16_moe / w4_a16_moe -- against (b) ops.w8_a16_moe_block / w4_a16_moe_block; the router formula alone against ops.moe_router;
and, at T <= 16, the fused router launch with tables (eetq_moe_router_f16) next to eetq_moe_route alone.  Both sides eager and both
captured as a HIP graph (one replay per timing); median of --iters with min and max.

    python tools/moe_bench.py --block --out <file>.jsonl
    python tools/moe_bench.py --block --bits 4 --out <file>.jsonl
(no output of this mode is committed under profiles/ yet: DESIGN.md 4.13)
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"mixtral-8x7b": (4096, 14336, 8, 2), "qwen3-30b-a3b": (2048, 768, 128, 8)}
# --block only (asked for by name): the sigmoid, group-limited rule; name -> (H, I, E, k), (n_group, topk_group, scale)
SIGMOID_SHAPES = {"deepseek-v3": ((7168, 2048, 256, 8), (8, 4, 2.5))}
DEV = "cuda:0"


def _time(fn, warmup, iters):
    return _time_stats(fn, warmup, iters)[0]


def _time_stats(fn, warmup, iters):
    """(median, min, max) us over `iters` launches"""
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
    return times[len(times) // 2], times[0], times[-1]


def _routing(T, k, E, kind, g):
    if kind == "uniform":
        return torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(DEV)
    # skewed: every token's first choice is expert 0
    rest = torch.stack([torch.randperm(E - 1, generator=g)[:k - 1] + 1 for _ in range(T)])
    return torch.cat([torch.zeros(T, 1, dtype=torch.long), rest], 1).to(DEV)


def _ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


def backward(args, out):
    import ctypes

    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd import _lib
    from eetq_amd.ops import w8_a16_gemm_t, w8_a16_moe, w8_a16_moe_backward, w8_a16_moe_train
    L = _lib.lib()
    for name in args.shapes.split(","):
        H, I, E, k = SHAPES[name]
        torch.manual_seed(0)
        gu_w = torch.randint(-127, 128, (E, H, 2 * I), dtype=torch.int8, device=DEV)
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-3).half()
        dn_w = torch.randint(-127, 128, (E, I, H), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-3).half()
        stacks = (gu_w, gu_s, dn_w, dn_s)
        cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=k)
        cfg._experts_implementation = "eager"
        eager = MixtralExperts(cfg).half().to(DEV)
        with torch.no_grad():
            eager.gate_up_proj.normal_(0, 0.02)
            eager.down_proj.normal_(0, 0.02)
        eager.requires_grad_(False)
        g = torch.Generator().manual_seed(1)
        for T in (int(t) for t in args.tokens.split(",")):
            S = T * k
            x = (torch.rand(T, H, device=DEV) - 0.5).half()
            idx = _routing(T, k, E, "uniform", g)
            wts = torch.rand(T, k, device=DEV).softmax(-1)
            dout = (torch.rand(T, H, device=DEV) - 0.5).half()
            active = torch.unique(idx).tolist()
            us_fwd = _time(lambda: w8_a16_moe(x, idx, wts, *stacks), args.warmup, args.iters)
            us_train = _time(lambda: w8_a16_moe_train(x, idx, wts, *stacks), args.warmup, args.iters)
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            o, tables, gate_up, y = w8_a16_moe_train(x, idx, wts, *stacks)
            torch.cuda.synchronize()
            saved = torch.cuda.memory_allocated() - m0 - o.numel() * 2
            us_bwd = _time(lambda: w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True), args.warmup, args.iters)
            torch.cuda.synchronize()
            m1 = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - m1
            # the five launches one at a time, on the tensors the backward makes
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            offsets, position = tables[E:], tables[2 * E + 1 + S:]
            active_t = tables[2 * E + 1 + 2 * S:]
            dy = torch.empty(S, H, dtype=torch.float16, device=DEV)
            dw = torch.empty_like(wts)
            dh = torch.empty(S, I, dtype=torch.float16, device=DEV)
            dgu = torch.empty(S, 2 * I, dtype=torch.float16, device=DEV)
            dxs = torch.empty(S, H, dtype=torch.float16, device=DEV)
            dx = torch.empty(T, H, dtype=torch.float16, device=DEV)
            ones = torch.ones(T, k, device=DEV)
            steps = {
                "combine_bwd": lambda: L.eetq_moe_combine_bwd_f16(_ptr(dout), _ptr(y), _ptr(position), _ptr(wts), 1, _ptr(dy),
                                                                  _ptr(dw), T, k, H, st),
                "gemm_t_down": lambda: L.eetq_w8a16_moe_gemm_t(_ptr(dy), _ptr(dn_w), _ptr(dn_s), _ptr(offsets), _ptr(active_t),
                                                               _ptr(dh), T, k, E, H, I, st),
                "silu_bwd": lambda: L.eetq_silu_mul_glu8_bwd_f16(_ptr(gate_up), _ptr(dh), _ptr(dgu), S, I, st),
                "gemm_t_gate_up": lambda: L.eetq_w8a16_moe_gemm_t(_ptr(dgu), _ptr(gu_w), _ptr(gu_s), _ptr(offsets),
                                                                  _ptr(active_t), _ptr(dxs), T, k, E, 2 * I, H, st),
                "combine": lambda: L.eetq_moe_combine_f16(_ptr(dxs), _ptr(position), _ptr(ones), 1, _ptr(dx), T, k, H, st),
            }
            split = {n: round(_time(f, args.warmup, args.iters), 2) for n, f in steps.items()}

            def loop():   # the workaround: host read-back, then per-expert w8_a16_gemm_t for both projections
                counts = tables[:E].cpu().tolist()
                off = 0
                for e in range(E):
                    c = counts[e]
                    if c:
                        w8_a16_gemm_t(dy[off:off + c], dn_w[e], dn_s[e])
                        w8_a16_gemm_t(dgu[off:off + c], gu_w[e], gu_s[e])
                        off += c
            us_loop = _time(loop, args.warmup, args.iters)
            xe = x.clone().requires_grad_()
            we = wts.clone().requires_grad_()

            def eager_fb():
                out_e = eager(xe, idx, we)
                out_e.backward(dout)
            us_eager = _time(eager_fb, max(1, args.warmup // 2), max(3, args.iters // 4))
            grouped = split["gemm_t_down"] + split["gemm_t_gate_up"]
            rec = {"shape": name, "H": H, "I": I, "E": E, "k": k, "T": T, "routing": "uniform", "active_experts": len(active),
                   "us_fwd_nograd": round(us_fwd, 2), "us_fwd_trainable": round(us_train, 2), "us_backward": round(us_bwd, 2),
                   "us_backward_split": split, "us_grouped_gemm_t": round(grouped, 2),
                   "us_per_expert_gemm_t_loop": round(us_loop, 2), "loop_over_grouped": round(us_loop / grouped, 2),
                   "bwd_over_trainable_fwd": round(us_bwd / us_train, 3),
                   "us_fp16_eager_fwd_bwd": round(us_eager, 2),
                   "saved_bytes": saved, "backward_peak_bytes": peak}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del o, tables, gate_up, y, dy, dh, dgu, dxs, dx


def _interleaved(fns, warmup, iters):
    """{name: (median, min, max) us}: the callables timed in turn, one call each per round, so that they share the device's state"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(iters):
        for n, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[n].append(a.elapsed_time(b) * 1000.0)
    return {n: (sorted(t)[len(t) // 2], min(t), max(t)) for n, t in times.items()}


def backward_i4(args, out):
    """the int4 training path next to the int8 backward on the same integers (expanded once, outside every timing)"""
    import ctypes

    from eetq_amd import _lib
    from eetq_amd.ops import w4_a16_moe, w4_a16_moe_backward, w4_a16_moe_path, w4_a16_moe_train, w8_a16_moe_backward
    L = _lib.lib()

    def r3(t):
        return [round(v, 2) for v in t]
    for name in args.shapes.split(","):
        H, I, E, k = SHAPES[name]
        torch.manual_seed(0)
        gu_w = torch.randint(-128, 128, (E, H, I), dtype=torch.int8, device=DEV)       # any bytes are valid int4 stacks
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-2).half()
        dn_w = torch.randint(-128, 128, (E, I, H // 2), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-2).half()
        stacks = (gu_w, gu_s, dn_w, dn_s)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        gu_w8 = torch.empty(E, H, 2 * I, dtype=torch.int8, device=DEV)
        dn_w8 = torch.empty(E, I, H, dtype=torch.int8, device=DEV)
        assert L.eetq_expand_i4_to_i8(_ptr(gu_w), _ptr(gu_w8), gu_w.numel(), st) == 0
        assert L.eetq_expand_i4_to_i8(_ptr(dn_w), _ptr(dn_w8), dn_w.numel(), st) == 0
        stacks8 = (gu_w8, gu_s, dn_w8, dn_s)
        g = torch.Generator().manual_seed(1)
        for T in (int(t) for t in args.tokens.split(",")):
            S = T * k
            x = (torch.rand(T, H, device=DEV) - 0.5).half()
            idx = _routing(T, k, E, "uniform", g)
            wts = torch.rand(T, k, device=DEV).softmax(-1)
            dout = (torch.rand(T, H, device=DEV) - 0.5).half()
            active = torch.unique(idx).tolist()
            fwd = _time_stats(lambda: w4_a16_moe(x, idx, wts, *stacks), args.warmup, args.iters)
            train = _time_stats(lambda: w4_a16_moe_train(x, idx, wts, *stacks), args.warmup, args.iters)
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            o, tables, gate_up, y = w4_a16_moe_train(x, idx, wts, *stacks)
            torch.cuda.synchronize()
            saved = torch.cuda.memory_allocated() - m0 - o.numel() * 2
            a4 = w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
            a8 = w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks8, True, True)
            assert torch.equal(a4[0], a8[0]) and torch.equal(a4[1], a8[1]), "int4 and int8 backward differ on the same integers"
            del a4, a8
            bwd = _interleaved({"int4": lambda: w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True),
                                "int8": lambda: w8_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks8, True, True)},
                               args.warmup, args.iters)
            torch.cuda.synchronize()
            m1 = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            w4_a16_moe_backward(dout, wts, tables, gate_up, y, *stacks, True, True)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - m1
            offsets, position = tables[E:], tables[2 * E + 1 + S:]
            active_t = tables[2 * E + 1 + 2 * S:]
            dy = torch.empty(S, H, dtype=torch.float16, device=DEV)
            dw = torch.empty_like(wts)
            dh = torch.empty(S, I, dtype=torch.float16, device=DEV)
            dgu = torch.empty(S, 2 * I, dtype=torch.float16, device=DEV)
            dxs = torch.empty(S, H, dtype=torch.float16, device=DEV)
            dx = torch.empty(T, H, dtype=torch.float16, device=DEV)
            ones = torch.ones(T, k, device=DEV)

            def gemm_t(fn, w, which):
                if which == "down":
                    return lambda: fn(_ptr(dy), _ptr(w), _ptr(dn_s), _ptr(offsets), _ptr(active_t), _ptr(dh), T, k, E, H, I, st)
                return lambda: fn(_ptr(dgu), _ptr(w), _ptr(gu_s), _ptr(offsets), _ptr(active_t), _ptr(dxs), T, k, E, 2 * I, H, st)
            split = {"combine_bwd": _time_stats(lambda: L.eetq_moe_combine_bwd_f16(_ptr(dout), _ptr(y), _ptr(position), _ptr(wts), 1,
                                                                                  _ptr(dy), _ptr(dw), T, k, H, st), args.warmup, args.iters)}
            down = _interleaved({"int4": gemm_t(L.eetq_w4a16_moe_gemm_t, dn_w, "down"),
                                 "int8": gemm_t(L.eetq_w8a16_moe_gemm_t, dn_w8, "down")}, args.warmup, args.iters)
            split["gemm_t_down"] = down["int4"]
            split["silu_bwd"] = _time_stats(lambda: L.eetq_silu_mul_glu8_bwd_f16(_ptr(gate_up), _ptr(dh), _ptr(dgu), S, I, st),
                                            args.warmup, args.iters)
            gate = _interleaved({"int4": gemm_t(L.eetq_w4a16_moe_gemm_t, gu_w, "gate_up"),
                                 "int8": gemm_t(L.eetq_w8a16_moe_gemm_t, gu_w8, "gate_up")}, args.warmup, args.iters)
            split["gemm_t_gate_up"] = gate["int4"]
            split["combine"] = _time_stats(lambda: L.eetq_moe_combine_f16(_ptr(dxs), _ptr(position), _ptr(ones), 1, _ptr(dx), T, k, H, st),
                                           args.warmup, args.iters)
            g4, g8 = down["int4"][0] + gate["int4"][0], down["int8"][0] + gate["int8"][0]
            rec = {"shape": name, "bits": 4, "H": H, "I": I, "E": E, "k": k, "T": T, "routing": "uniform", "active_experts": len(active),
                   "iters": args.iters, "fwd_path": w4_a16_moe_path(T, k, E, H, I), "us_fwd_nograd": r3(fwd), "us_fwd_trainable": r3(train),
                   "us_backward": r3(bwd["int4"]), "us_backward_int8_same_integers": r3(bwd["int8"]),
                   "backward_int4_over_int8": round(bwd["int4"][0] / bwd["int8"][0], 3),
                   "us_backward_split": {n: r3(t) for n, t in split.items()},
                   "us_gemm_t_down_int8": r3(down["int8"]), "us_gemm_t_gate_up_int8": r3(gate["int8"]),
                   "gemm_t_down_int4_over_int8": round(down["int4"][0] / down["int8"][0], 3),
                   "gemm_t_gate_up_int4_over_int8": round(gate["int4"][0] / gate["int8"][0], 3),
                   "gemm_t_pair_int4_over_int8": round(g4 / g8, 3),
                   "bwd_over_trainable_fwd": round(bwd["int4"][0] / train[0], 3),
                   "saved_bytes": saved, "backward_peak_bytes": peak}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del o, tables, gate_up, y, dy, dh, dgu, dxs, dx


def seam(args, out):
    import ctypes

    from eetq_amd import _lib
    L = _lib.lib()
    for name in args.shapes.split(","):
        H, I, E, k = SHAPES[name]
        torch.manual_seed(0)
        gu_w = torch.randint(-127, 128, (E, H, 2 * I), dtype=torch.int8, device=DEV)
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-3).half()
        dn_w = torch.randint(-127, 128, (E, I, H), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-3).half()
        g = torch.Generator().manual_seed(1)
        done = set()
        for rows in (int(r) for r in args.seam_rows.split(",")):
            T = max(17, rows * E // k)   # the prompt path starts at T = 17
            if T in done:
                continue
            done.add(T)
            S, A = T * k, min(E, T * k)
            for kind in ("uniform", "skewed"):
                x = (torch.rand(T, H, device=DEV) - 0.5).half()
                idx = _routing(T, k, E, kind, g)
                tabs = [torch.empty(n, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)]
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                assert L.eetq_moe_route(_ptr(idx), T, k, E, *[_ptr(t) for t in tabs], st) == 0
                _, offsets, sorted_slot, _, active = tabs
                inter = torch.empty(S, I, dtype=torch.float16, device=DEV)
                down = torch.empty(S, H, dtype=torch.float16, device=DEV)
                tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))

                def pair(fn):
                    a = fn(_ptr(x), _ptr(gu_w), _ptr(gu_s), *tab, _ptr(inter), T, k, E, 2 * I, H, 1, 1, st)
                    b = fn(_ptr(inter), _ptr(dn_w), _ptr(dn_s), *tab, _ptr(down), T, k, E, H, I, 0, 0, st)
                    assert a == 0 and b == 0, (a, b)
                us_dec = _time(lambda: pair(L.eetq_w8a16_moe_gemm), args.warmup, args.iters)
                us_tile = _time(lambda: pair(L.eetq_w8a16_moe_gemm_tiled), args.warmup, args.iters)
                rec = {"shape": name, "H": H, "I": I, "E": E, "k": k, "T": T, "mean_rows": round(S / E, 2), "routing": kind,
                       "max_rows": int(tabs[0].max()), "us_decode_kernel": round(us_dec, 2), "us_tiled_kernel": round(us_tile, 2),
                       "decode_over_tiled": round(us_dec / us_tile, 3)}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()


def seam_i4(args, out):
    """the int4 layer's two routes per pair of projections: the decode kernel on the int4 tiles vs expansion + the tiled kernel"""
    import ctypes

    from eetq_amd import _lib
    L = _lib.lib()
    for name in args.shapes.split(","):
        H, I, E, k = SHAPES[name]
        torch.manual_seed(0)
        gu_w = torch.randint(-128, 128, (E, H, I), dtype=torch.int8, device=DEV)
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-2).half()
        dn_w = torch.randint(-128, 128, (E, I, H // 2), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-2).half()
        w8 = torch.empty(E * H * 2 * I, dtype=torch.int8, device=DEV)   # one projection's expansion at a time, like the layer
        g = torch.Generator().manual_seed(1)
        done = set()
        for rows in (int(r) for r in args.seam_rows.split(",")):
            T = max(17, rows * E // k)
            if T in done:
                continue
            done.add(T)
            S, A = T * k, min(E, T * k)
            for kind in ("uniform", "skewed"):
                x = (torch.rand(T, H, device=DEV) - 0.5).half()
                idx = _routing(T, k, E, kind, g)
                tabs = [torch.empty(n, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)]
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                assert L.eetq_moe_route(_ptr(idx), T, k, E, *[_ptr(t) for t in tabs], st) == 0
                _, offsets, sorted_slot, _, active = tabs
                inter = torch.empty(S, I, dtype=torch.float16, device=DEV)
                down = torch.empty(S, H, dtype=torch.float16, device=DEV)
                tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))

                def decode():
                    a = L.eetq_w4a16_moe_gemm(_ptr(x), _ptr(gu_w), _ptr(gu_s), *tab, _ptr(inter), T, k, E, 2 * I, H, 1, 1, st)
                    b = L.eetq_w4a16_moe_gemm(_ptr(inter), _ptr(dn_w), _ptr(dn_s), *tab, _ptr(down), T, k, E, H, I, 0, 0, st)
                    assert a == 0 and b == 0, (a, b)

                def expand_only():
                    a = L.eetq_expand_i4_to_i8(_ptr(gu_w), _ptr(w8), gu_w.numel(), st)
                    b = L.eetq_expand_i4_to_i8(_ptr(dn_w), _ptr(w8), dn_w.numel(), st)
                    assert a == 0 and b == 0, (a, b)

                def expanded():
                    a = L.eetq_expand_i4_to_i8(_ptr(gu_w), _ptr(w8), gu_w.numel(), st)
                    b = L.eetq_w8a16_moe_gemm_tiled(_ptr(x), _ptr(w8), _ptr(gu_s), *tab, _ptr(inter), T, k, E, 2 * I, H, 1, 1, st)
                    c = L.eetq_expand_i4_to_i8(_ptr(dn_w), _ptr(w8), dn_w.numel(), st)
                    d = L.eetq_w8a16_moe_gemm_tiled(_ptr(inter), _ptr(w8), _ptr(dn_s), *tab, _ptr(down), T, k, E, H, I, 0, 0, st)
                    assert a == 0 and b == 0 and c == 0 and d == 0, (a, b, c, d)

                def direct():
                    a = L.eetq_w4a16_moe_gemm_tiled(_ptr(x), _ptr(gu_w), _ptr(gu_s), *tab, _ptr(inter), T, k, E, 2 * I, H, 1, 1, 0, st)
                    b = L.eetq_w4a16_moe_gemm_tiled(_ptr(inter), _ptr(dn_w), _ptr(dn_s), *tab, _ptr(down), T, k, E, H, I, 0, 0, 0, st)
                    assert a == 0 and b == 0, (a, b)
                us_dec, dec_lo, dec_hi = _time_stats(decode, args.warmup, args.iters)
                us_exp, exp_lo, exp_hi = _time_stats(expanded, args.warmup, args.iters)
                us_only = _time(expand_only, args.warmup, args.iters)
                rec = {"shape": name, "bits": 4, "H": H, "I": I, "E": E, "k": k, "T": T, "mean_rows": round(S / E, 2), "routing": kind,
                       "max_rows": int(tabs[0].max()), "us_decode_kernel": round(us_dec, 2), "us_expand_plus_tiled": round(us_exp, 2),
                       "us_expansions_alone": round(us_only, 2), "decode_over_expanded": round(us_dec / us_exp, 3)}
                if args.path == "direct":
                    us_dir, lo, hi = _time_stats(direct, args.warmup, args.iters)
                    rec.update({"us_direct": round(us_dir, 2), "us_direct_min": round(lo, 2), "us_direct_max": round(hi, 2),
                                "us_decode_min_max": [round(dec_lo, 2), round(dec_hi, 2)],
                                "us_expand_min_max": [round(exp_lo, 2), round(exp_hi, 2)],
                                "decode_over_direct": round(us_dec / us_dir, 3), "expanded_over_direct": round(us_exp / us_dir, 3)})
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()


PLANS = ("8x2", "4x1", "2x1")


def _graphed(fn):
    """fn captured once (after a warm-up call) -> a callable that replays the graph"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    g.keep = keep
    return g.replay


def block(args, out):
    """the whole sparse block: torch router + layer op (the sequence before DESIGN.md 4.13) against the block op"""
    import ctypes

    import torch.nn.functional as F

    from eetq_amd import _lib, ops
    lib = _lib.lib()
    for name in args.shapes.split(","):
        sigmoid = SIGMOID_SHAPES.get(name)
        H, I, E, k = sigmoid[0] if sigmoid else SHAPES[name]
        torch.manual_seed(0)
        pack = 2 if args.bits == 4 else 1
        gu_w = torch.randint(-127, 128, (E, H, 2 * I // pack), dtype=torch.int8, device=DEV)
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-3).half()
        dn_w = torch.randint(-127, 128, (E, I, H // pack), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-3).half()
        stacks = (gu_w, gu_s, dn_w, dn_s)
        layer = ops.w4_a16_moe if args.bits == 4 else ops.w8_a16_moe
        block_op = ops.w4_a16_moe_block if args.bits == 4 else ops.w8_a16_moe_block
        mixtral = name.startswith("mixtral")   # fp32 scores, always renormalised; the others: fp16 scores
        sdt = torch.float32 if mixtral else torch.float16
        wr = (torch.randn(E, H, device=DEV) / H ** 0.5).half()

        def torch_router(x):
            logits = F.linear(x, wr)
            top, idx = torch.topk(F.softmax(logits, dtype=torch.float, dim=-1), k, dim=-1)
            top /= top.sum(dim=-1, keepdim=True)
            return logits, top.to(sdt), idx

        if sigmoid:
            G, KG, scale = sigmoid[1]
            sdt = torch.float32
            bias = (torch.rand(E, device=DEV) * 0.5 - 0.25).half()
            rule = (bias, k, G, KG, True, scale)
            block_op = ops.w4_a16_moe_block_sigmoid if args.bits == 4 else ops.w8_a16_moe_block_sigmoid

            def torch_router(x):  # noqa: F811 -- DeepseekV3TopkRouter.forward, op for op
                logits = F.linear(x.type(torch.float32), wr.type(torch.float32))
                scores = logits.sigmoid()
                choice = scores + bias
                group_scores = choice.view(-1, G, E // G).topk(2, dim=-1)[0].sum(dim=-1)
                group_idx = torch.topk(group_scores, k=KG, dim=-1, sorted=False)[1]
                group_mask = torch.zeros_like(group_scores)
                group_mask.scatter_(1, group_idx, 1)
                score_mask = group_mask.unsqueeze(-1).expand(-1, G, E // G).reshape(-1, E)
                choice = choice.masked_fill(~score_mask.bool(), float("-inf"))
                idx = torch.topk(choice, k=k, dim=-1, sorted=False)[1]
                top = scores.gather(1, idx)
                top /= top.sum(dim=-1, keepdim=True) + 1e-20
                return logits, top * scale, idx

        for T in (int(t) for t in args.tokens.split(",")):
            x = torch.randn(T, H, device=DEV).half()

            def before():
                _, sc, idx = torch_router(x)
                return layer(x, idx, sc, *stacks)

            def after():
                return block_op(x, wr, *rule, *stacks) if sigmoid else block_op(x, wr, k, True, sdt, *stacks)

            def router_op():
                return ops.moe_router_sigmoid(x, wr, *rule) if sigmoid else ops.moe_router(x, wr, k, True, sdt)

            cases = {"before": before, "after": after, "router_torch": lambda: torch_router(x), "router_op": router_op}
            if T <= 16 and not sigmoid:
                S, A = T * k, min(E, T * k)
                lg = torch.empty(T, E, dtype=torch.float16, device=DEV)
                ix = torch.zeros(T, k, dtype=torch.int64, device=DEV)
                sc = torch.empty(T, k, dtype=sdt, device=DEV)
                tb = [torch.empty(n, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)]
                st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                dt = 1 if sdt == torch.float32 else 0
                cases["router_launch_with_tables"] = lambda: lib.eetq_moe_router_f16(
                    _ptr(x), _ptr(wr), T, H, E, k, 1, dt, _ptr(lg), _ptr(ix), _ptr(sc), *[_ptr(t) for t in tb], st)
                cases["route_launch"] = lambda: lib.eetq_moe_route(_ptr(ix), T, k, E, *[_ptr(t) for t in tb], st)
            with torch.no_grad():
                assert torch.equal(after(), layer(x, *router_op()[2:0:-1], *stacks))
                rec = {"shape": name, "bits": args.bits, "T": T, "H": H, "I": I, "E": E, "k": k, "iters": args.iters}
                for tag, fn in cases.items():
                    for mode, f in (("eager", fn), ("graph", _graphed(fn) if "launch" not in tag else None)):
                        if f is None:
                            continue
                        med, lo, hi = _time_stats(f, args.warmup, args.iters)
                        rec["us_%s_%s" % (tag, mode)] = [round(med, 2), round(lo, 2), round(hi, 2)]
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


def plan_child(args):
    """one process = one forced plan (or none): us of eetq_w4a16_moe_gemm per projection at T = 1, 4, 16, uniform routing"""
    import ctypes

    from eetq_amd import _lib
    L = _lib.lib()
    plan = os.environ.get("EETQ_AMD_MOE_I4_PLAN", "default")
    for name in args.shapes.split(","):
        H, I, E, k = SHAPES[name]
        torch.manual_seed(0)
        gu_w = torch.randint(-128, 128, (E, H, I), dtype=torch.int8, device=DEV)
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-2).half()
        dn_w = torch.randint(-128, 128, (E, I, H // 2), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-2).half()
        g = torch.Generator().manual_seed(1)
        for T in (1, 4, 16):
            S, A = T * k, min(E, T * k)
            x = (torch.rand(T, H, device=DEV) - 0.5).half()
            idx = _routing(T, k, E, "uniform", g)
            tabs = [torch.empty(n, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, A)]
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            assert L.eetq_moe_route(_ptr(idx), T, k, E, *[_ptr(t) for t in tabs], st) == 0
            _, offsets, sorted_slot, _, active = tabs
            inter = torch.zeros(S, I, dtype=torch.float16, device=DEV)
            down = torch.empty(S, H, dtype=torch.float16, device=DEV)
            tab = (_ptr(offsets), _ptr(sorted_slot), _ptr(active))
            for proj, fn, K in (("gate_up", lambda: L.eetq_w4a16_moe_gemm(_ptr(x), _ptr(gu_w), _ptr(gu_s), *tab, _ptr(inter), T, k, E,
                                                                          2 * I, H, 1, 1, st), H),
                                ("down", lambda: L.eetq_w4a16_moe_gemm(_ptr(inter), _ptr(dn_w), _ptr(dn_s), *tab, _ptr(down), T, k, E,
                                                                       H, I, 0, 0, st), I)):
                wv, d = (int(v) for v in plan.split("x")) if plan != "default" else (0, 0)
                us, lo, hi = _time_stats(fn, args.warmup, args.iters)
                print(json.dumps({"shape": name, "proj": proj, "K": K, "k_tiles": K // 128, "T": T, "plan": plan,
                                  "plan_applied": plan == "default" or K // 128 >= wv * d, "us": round(us, 2), "us_min": round(lo, 2),
                                  "us_max": round(hi, 2)}), flush=True)


def plan_sweep(args, out):
    for plan in ("default",) + PLANS:
        env = dict(os.environ)
        if plan != "default":
            env.update(EETQ_AMD_TUNING="1", EETQ_AMD_MOE_I4_PLAN=plan)
        cmd = [sys.executable, os.path.abspath(__file__), "--plan-child", "--shapes", args.shapes, "--warmup", str(args.warmup),
               "--iters", str(args.iters)]
        res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True)
        for line in res.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()


def _host_path_times(args):
    """{(shape, T, routing): us} of the layer on the host path, from a child process that sets the A/B switch"""
    env = dict(os.environ, EETQ_AMD_TUNING="1", EETQ_AMD_MOE_HOST="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--shapes", args.shapes, "--tokens", args.tokens, "--warmup", str(args.warmup),
           "--iters", str(args.iters), "--no-baselines"]
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, check=True)
    times = {}
    for line in res.stdout.splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            assert r["path"] == "host" or r["T"] <= 16, r
            times[(r["shape"], r["T"], r["routing"])] = (r["us"], r["us_min"], r["us_max"])
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--tokens", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--backward", action="store_true", help="time the training path (DESIGN.md 4.11)")
    ap.add_argument("--host-path", action="store_true", help="add us_host_path: the T > 16 host path, timed in a child process")
    ap.add_argument("--no-baselines", action="store_true", help="skip the fp16 eager forward and the per-expert Python loop")
    ap.add_argument("--seam", action="store_true", help="sweep the seam between the two grouped kernels (DESIGN.md 4.10)")
    ap.add_argument("--seam-rows", default=None,
                    help="mean rows per expert of the seam sweep (default 1,2,4,8,16,32,64; 16,32,64,128,256 with --bits 4)")
    ap.add_argument("--bits", type=int, choices=(8, 4), default=8, help="the layer table / --seam on int8 or int4 expert stacks")
    ap.add_argument("--path", choices=("auto", "direct"), default="auto",
                    help="--bits 4: 'direct' = the grouped tiled kernel on the int4 tiles (DESIGN.md 4.12), in the layer table and --seam")
    ap.add_argument("--plan-sweep", action="store_true", help="sweep eetq_w4a16_moe_gemm's instantiations (DESIGN.md 4.12)")
    ap.add_argument("--plan-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--block", action="store_true", help="time the whole sparse block with and without the device router (DESIGN.md 4.13)")
    args = ap.parse_args()
    if args.path != "auto" and args.bits != 4:
        ap.error("--path direct needs --bits 4")
    if args.block:
        args.tokens = args.tokens or "1,4,16,64,512"
        out = open(args.out, "w") if args.out else None
        block(args, out)
        if out:
            out.close()
        return
    if args.plan_child:
        plan_child(args)
        return
    if args.plan_sweep:
        out = open(args.out, "w") if args.out else None
        plan_sweep(args, out)
        if out:
            out.close()
        return
    if args.seam:
        args.seam_rows = args.seam_rows or ("16,32,64,128,256" if args.bits == 4 else "1,2,4,8,16,32,64")
        out = open(args.out, "w") if args.out else None
        (seam_i4 if args.bits == 4 else seam)(args, out)
        if out:
            out.close()
        return
    if args.backward:
        args.tokens = args.tokens or "16,64,512,4096"
        out = open(args.out, "w") if args.out else None
        (backward_i4 if args.bits == 4 else backward)(args, out)
        if out:
            out.close()
        return
    args.tokens = args.tokens or "1,2,4,8,16,64,512,4096"
    host_us = _host_path_times(args) if args.host_path else {}   # before this process opens the GPU

    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    from eetq_amd import _lib
    from eetq_amd.ops import w4_a16_moe, w4_a16_moe_direct_supported, w4_a16_moe_path, w8_a16_gemm, w8_a16_moe
    if args.bits == 4:
        args.no_baselines = True
    host = _lib.lib().eetq_diag_moe_host_path() == 1
    out = open(args.out, "w") if args.out else None
    for name in args.shapes.split(","):
        H, I, E, k = SHAPES[name]
        torch.manual_seed(0)
        gu_w = torch.randint(-127, 128, (E, H, 2 * I), dtype=torch.int8, device=DEV)
        gu_s = (torch.rand(E, 2 * I, device=DEV) * 1e-3).half()
        dn_w = torch.randint(-127, 128, (E, I, H), dtype=torch.int8, device=DEV)
        dn_s = (torch.rand(E, H, device=DEV) * 1e-3).half()
        if args.bits == 4:   # any bytes are valid int4 stacks: [E, H, I] and [E, I, H / 2]
            gu_w = torch.randint(-128, 128, (E, H, I), dtype=torch.int8, device=DEV)
            dn_w = torch.randint(-128, 128, (E, I, H // 2), dtype=torch.int8, device=DEV)
        layer = w4_a16_moe if args.bits == 4 else w8_a16_moe
        if not args.no_baselines:
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

                # --path direct: the module's opt-in rule (T > 16, T k >= 16 E, both projections supported), else the decode kernel
                direct = (args.path == "direct" and T > 16 and T * k >= 16 * E and w4_a16_moe_direct_supported(T, k, E, H, I))
                extra = () if args.path == "auto" else ("direct" if direct else "decode",)
                us, us_lo, us_hi = _time_stats(lambda: layer(x, idx, wts, gu_w, gu_s, dn_w, dn_s, *extra), args.warmup, args.iters)
                nbytes = len(active) * 3 * H * I * args.bits // 8
                rec = {"shape": name, "H": H, "I": I, "E": E, "k": k, "T": T, "routing": kind, "active_experts": len(active),
                       "path": "host" if host and T > 16 else "device", "us": round(us, 2), "us_min": round(us_lo, 2),
                       "us_max": round(us_hi, 2), "bits": args.bits, "int8_bytes" if args.bits == 8 else "int4_bytes": nbytes,
                       "TBps": round(nbytes / us / 1e6, 3), "TFLOPs": round(6.0 * T * k * H * I / us / 1e6, 1)}
                if args.bits == 4:
                    rec["path"] = extra[0] if extra else w4_a16_moe_path(T, k, E, H, I)
                if (name, T, kind) in host_us:
                    rec["us_host_path"], rec["us_host_path_min"], rec["us_host_path_max"] = host_us[(name, T, kind)]
                    rec["host_over_device"] = round(rec["us_host_path"] / us, 2)
                if not args.no_baselines:
                    with torch.no_grad():
                        us_eager = _time(lambda: eager(x, idx, wts), args.warmup, args.iters)
                    us_loop = _time(loop, args.warmup, args.iters)
                    rec.update({"us_fp16_eager": round(us_eager, 2), "us_per_expert_loop": round(us_loop, 2),
                                "speedup_vs_eager": round(us_eager / us, 2)})
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
