"""Decode-step attention at Llama-2-13B shapes (40 heads x 128, one new token), as the graph decoder issues it: `layers`
independent caches (together larger than the 256 MB Infinity Cache) stepped back to back inside one HIP graph.
Prints microseconds per layer-step for the one-launch form (eetq_rope_decode_attention_f16) over a sweep of chunk counts,
and for the two-launch pair.  usage: python tools/attn_bench.py [--filled 1024] [--rows 1082] [--batch 1]
--kv-bits 8: the same sweep over an int8 KV cache (eetq_rope_decode_attention_i8kv_f16).  --compare-lib PATH: one process alternates
the fp16 one-launch form of the library at PATH (e.g. the parent commit's build), this tree's fp16 form and its int8 form, --rounds
times each, at the default chunk count.  --write T: the prompt's cache write at T tokens, fp16 against the quantising int8 write."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eetq_amd.ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--filled", type=int, default=1024)
ap.add_argument("--rows", type=int, default=1082)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--kv-heads", type=int, default=40)
ap.add_argument("--layers", type=int, default=20)
ap.add_argument("--splits", default="default,4,8,12,17,25,34")
ap.add_argument("--stamps", action="store_true", help="per-phase device-clock decomposition of the one-launch form")
ap.add_argument("--stamps-fused", action="store_true", help="device-clock decomposition of the fused attention + o projection launch")
ap.add_argument("--pair", action="store_true", help="attention + the o projection behind it (H*D x H*D int8), with and without "
                                                    "the L2 prefetch of the projection's weight inside the attention launch")
ap.add_argument("--kv-bits", type=int, default=16, choices=(16, 8), help="8: an int8 KV cache with a scale pair per row")
ap.add_argument("--compare-lib", default=None, help="another build of libeetq_amd.so to alternate with (its fp16 one-launch form)")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--write", type=int, default=0, help="time the prompt cache write at this many tokens instead (fp16 and int8)")
args = ap.parse_args()
if args.kv_bits == 8 and (args.stamps or args.stamps_fused or args.pair):
    sys.exit("--kv-bits 8 goes with the chunk sweep, --compare-lib and --write only")
dev = "cuda:0"
B, H, Hkv, D, S, L = args.batch, args.heads, args.kv_heads, 128, args.rows, args.layers
torch.manual_seed(0)
inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
fr = torch.einsum("i,j->ij", torch.arange(S + 64).float(), inv)
table = torch.cat([fr.cos(), fr.sin()], -1).half().to(dev)
want16 = args.kv_bits == 16 or args.compare_lib is not None or args.write > 0
want8 = args.kv_bits == 8 or args.compare_lib is not None or args.write > 0
kc = [torch.randn(B, Hkv, S, D, dtype=torch.float16, device=dev) for _ in range(L if want16 else 0)]
vc = [torch.randn(B, Hkv, S, D, dtype=torch.float16, device=dev) for _ in range(L if want16 else 0)]
# int8 rows: bytes uniform in [-127, 127], scales near 1 / 42 (an N(0, 1) row of 128 values has an absmax near 3)
kc8 = [torch.randint(-127, 128, (B, Hkv, S, D), dtype=torch.int8, device=dev) for _ in range(L if want8 else 0)]
vc8 = [torch.randint(-127, 128, (B, Hkv, S, D), dtype=torch.int8, device=dev) for _ in range(L if want8 else 0)]
sc8 = [(torch.rand(B, Hkv, S, 2, device=dev) * 0.01 + 0.02).half() for _ in range(L if want8 else 0)]
qkv = torch.randn(B, 1, (H + 2 * Hkv) * D, dtype=torch.float16, device=dev)
q = qkv[..., : H * D].unflatten(-1, (H, D))[:, 0]
k = qkv[..., H * D: (H + Hkv) * D].unflatten(-1, (Hkv, D))[:, 0]
v = qkv[..., (H + Hkv) * D:].unflatten(-1, (Hkv, D))[:, 0]
pos = torch.full((B,), args.filled, dtype=torch.int64, device=dev)
tickets = [torch.zeros(B * H + 1, dtype=torch.int32, device=dev) for _ in range(L)]
counters = [torch.tensor(args.filled, dtype=torch.int64, device=dev) for _ in range(L)]
kv_mb = 2 * B * Hkv * (args.filled + 1) * D * 2 / 1e6            # fp16: 4 D bytes per row (K and V)
kv8_mb = B * Hkv * (args.filled + 1) * (2 * D + 4) / 1e6         # int8: 2 D + 4


def one_launch(i, splits):
    return ops.rope_decode_attention(pos, q, k, v, table, kc[i], vc[i], tickets[i], slots=counters[i], splits=splits,
                                     kv_len=counters[i], kv_len_bias=1)


def two_launch(i, splits):
    ops.rotary_embedding_neox_kvcache(pos, q, k, v, D, table, kc[i], vc[i], slots=counters[i])
    return ops.decode_attention(q, kc[i], vc[i], splits=splits, kv_len=counters[i], kv_len_bias=1)


def one_launch_i8(i, splits):
    return ops.rope_decode_attention_i8kv(pos, q, k, v, table, kc8[i], vc8[i], sc8[i], tickets[i], slots=counters[i], splits=splits,
                                          kv_len=counters[i], kv_len_bias=1)


def two_launch_i8(i, splits):
    ops.rotary_embedding_neox_kvcache_prefill_i8(pos[:, None], q[:, None], k[:, None], v[:, None], D, table, kc8[i], vc8[i], sc8[i],
                                                 first_row_dev=counters[i])
    return ops.decode_attention_i8kv(q, kc8[i], vc8[i], sc8[i], splits=splits, kv_len=counters[i], kv_len_bias=1)


def timed(fn, splits, reps=30):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(L):
            fn(i, splits)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(L):
                fn(i, splits)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * L)


def record(form, lib, bits, s, us):
    mb = kv_mb if bits == 16 else kv8_mb
    print(json.dumps({"form": form, "lib": lib, "kv_bits": bits, "splits": s, "batch": B, "heads": H, "kv_heads": Hkv,
                      "filled": args.filled, "rows": S, "us_per_layer_step": round(us, 2), "kv_MB": round(mb, 1),
                      "kv_GBps": round(mb / us * 1e3, 0)}), flush=True)


if args.write:
    T = args.write
    wide = torch.randn(B, T, (H + 2 * Hkv) * D, dtype=torch.float16, device=dev)
    wq = wide[..., : H * D].unflatten(-1, (H, D))
    wk = wide[..., H * D: (H + Hkv) * D].unflatten(-1, (Hkv, D))
    wv = wide[..., (H + Hkv) * D:].unflatten(-1, (Hkv, D))
    wpos = torch.arange(T, device=dev).repeat(B, 1).contiguous()

    def write16(i, _):
        ops.rotary_embedding_neox_kvcache_prefill(wpos, wq, wk, wv, D, table, kc[i], vc[i])

    def write8(i, _):
        ops.rotary_embedding_neox_kvcache_prefill_i8(wpos, wq, wk, wv, D, table, kc8[i], vc8[i], sc8[i])

    for rnd in range(args.rounds):
        for name, fn, bits in (("prompt_write", write16, 16), ("prompt_write", write8, 8)):
            print(json.dumps({"form": name, "kv_bits": bits, "tokens": T, "batch": B, "heads": H, "kv_heads": Hkv, "round": rnd,
                              "us_per_layer": round(timed(fn, None), 2)}), flush=True)
    sys.exit(0)

if args.compare_lib:
    import ctypes
    from eetq_amd import _lib
    mine = _lib.lib()
    other = ctypes.CDLL(os.path.abspath(args.compare_lib))
    for name in ("eetq_rope_decode_attention_bounded_f16", "eetq_decode_attention_splits"):
        getattr(other, name).argtypes = getattr(mine, name).argtypes
        getattr(other, name).restype = ctypes.c_int
    splits = other.eetq_decode_attention_splits(B, H, S)
    assert splits == mine.eetq_decode_attention_splits(B, H, S)
    out_o = torch.empty(B, H, D, dtype=torch.float16, device=dev)
    ws_o = torch.empty(B * H * splits * (D + 4), dtype=torch.float32, device=dev)

    def other_one_launch(i, _):
        st = (ctypes.c_long * 12)(q.stride(0), k.stride(0), v.stride(0), kc[i].stride(0), kc[i].stride(1), kc[i].stride(2),
                                  vc[i].stride(0), vc[i].stride(1), vc[i].stride(2), 0, out_o.stride(0), out_o.stride(1))
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        rc = other.eetq_rope_decode_attention_bounded_f16(
            p(pos), p(counters[i]), 0, p(q), p(k), p(v), p(table), table.shape[0], p(kc[i]), p(vc[i]), None, p(out_o), p(ws_o),
            p(tickets[i]), B, H, Hkv, S, D, splits, D ** -0.5, st, p(counters[i]), 1, None,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        return out_o

    same = bool(torch.equal(other_one_launch(0, None).clone(), one_launch(0, splits)))
    print(json.dumps({"compare_lib": args.compare_lib, "fp16_same_bits_as_compare_lib": same, "splits": splits}), flush=True)
    for rnd in range(args.rounds):
        record("one_launch", "compare", 16, "default", timed(other_one_launch, None))
        record("one_launch", "tree", 16, "default", timed(one_launch, None))
        record("one_launch", "tree", 8, "default", timed(one_launch_i8, None))
    sys.exit(0)

if args.pair:
    C = H * D
    gw = torch.Generator(device=dev).manual_seed(3)
    ow = [torch.randint(-128, 127, (C, C), dtype=torch.int8, device=dev, generator=gw) for _ in range(L)]
    osc = [(torch.rand(C, dtype=torch.float16, device=dev, generator=gw) * 0.01 + 0.001) for _ in range(L)]
    res = torch.zeros(B, C, dtype=torch.float16, device=dev)

    def pair(i, hint):
        kw = {"next_weight": ow[i]} if hint else {}   # (the hint exists only with tools/experiments/attn_l2_prefetch.patch applied)
        att = ops.rope_decode_attention(pos, q, k, v, table, kc[i], vc[i], tickets[i], slots=counters[i], kv_len=counters[i],
                                        kv_len_bias=1, **kw)
        return ops.w8_a16_gemm(att.view(B, C), ow[i], osc[i], residual=res)

    def attn_only(i, _):
        return ops.rope_decode_attention(pos, q, k, v, table, kc[i], vc[i], tickets[i], slots=counters[i], kv_len=counters[i], kv_len_bias=1)

    def attn_hint_only(i, _):
        return ops.rope_decode_attention(pos, q, k, v, table, kc[i], vc[i], tickets[i], slots=counters[i], kv_len=counters[i], kv_len_bias=1,
                                         next_weight=ow[i])

    try:
        attn_hint_only(0, None)
        have_hint = True
    except TypeError:
        have_hint = False

    def proj_only(i, _):
        return ops.w8_a16_gemm(res, ow[i], osc[i], residual=res)

    tickets2 = [torch.zeros(ops.rope_decode_attention_oproj_tickets(H) if getattr(ops, 'rope_decode_attention_oproj_tickets', None) else B * H + 2, dtype=torch.int32, device=dev) for _ in range(L)]
    have_fused = (getattr(ops, "rope_decode_attention_oproj", None) is not None and B == 1
                  and ops.rope_decode_attention_oproj_supported(1, H, D, C, False))

    def fused(i, _):
        return ops.rope_decode_attention_oproj(pos, q, k, v, table, kc[i], vc[i], tickets2[i], ow[i], osc[i], None, res.view(-1),
                                               slots=counters[i], kv_len=counters[i], kv_len_bias=1)

    y0 = pair(0, False).clone()
    same = bool(torch.equal(y0, pair(0, True).clone())) if have_hint else None
    out = {"form": "attention + o projection", "batch": B, "heads": H, "filled": args.filled, "rows": S, "o_proj": "%dx%d" % (C, C),
           "same_bits_with_hint": same}
    if have_fused:
        yf = fused(0, None).clone().view(B, C)
        torch.cuda.synchronize()
        err = (yf.float() - y0.float()).abs().max().item()
        out["fused_vs_pair_max_abs"] = err
        out["fused_vs_pair_tier_a"] = bool(((yf.float() - y0.float()).abs() <= 1e-3 * y0.float().abs().max() + 2e-3 * y0.float().abs()).all())
        out["fused_timeouts"] = ops.attn_oproj_timeouts()
    for rep in range(2):
        out["attention_us"] = round(timed(attn_only, None), 2)
        if have_hint:
            out["attention_with_prefetch_us"] = round(timed(attn_hint_only, None), 2)
        out["o_proj_us"] = round(timed(proj_only, None), 2)
        out["pair_us"] = round(timed(pair, False), 2)
        if have_hint:
            out["pair_with_prefetch_us"] = round(timed(pair, True), 2)
        if have_fused:
            out["fused_us"] = round(timed(fused, None), 2)
            out["fused_timeouts_after"] = ops.attn_oproj_timeouts()
        print(json.dumps(out), flush=True)
    sys.exit(0)

if args.stamps_fused:
    import ctypes
    from eetq_amd import _lib
    lib = _lib.lib()
    C = H * D
    gw = torch.Generator(device=dev).manual_seed(3)
    ow = [torch.randint(-128, 127, (C, C), dtype=torch.int8, device=dev, generator=gw) for _ in range(L)]
    osc = [(torch.rand(C, dtype=torch.float16, device=dev, generator=gw) * 0.01 + 0.001) for _ in range(L)]
    res = torch.zeros(B, C, dtype=torch.float16, device=dev)
    tk = [torch.zeros(ops.rope_decode_attention_oproj_tickets(H), dtype=torch.int32, device=dev) for _ in range(L)]
    splits = lib.eetq_decode_attention_splits(B, H, S)
    A, R = H * splits, C // 16
    buf = torch.zeros((A + R) * 8, dtype=torch.int64, device=dev)

    def fused(i):
        return ops.rope_decode_attention_oproj(pos, q, k, v, table, kc[i], vc[i], tk[i], ow[i], osc[i], None, res.view(-1),
                                               slots=counters[i], kv_len=counters[i], kv_len_bias=1)

    lib.eetq_diag_attn_stamps(ctypes.c_void_p(buf.data_ptr()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(L):
            fused(i)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(L):
                fused(i)
    torch.cuda.current_stream().wait_stream(side)
    lib.eetq_diag_attn_stamps(None)
    rows = []
    for it in range(12):
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        st = buf.view(A + R, 8).cpu().double()
        t0 = st[:, 0][st[:, 0] > 0].min()
        rel = (st - t0) / 100.0
        rel[st == 0] = float("nan")
        rows.append(rel)
    allr = torch.stack(rows[2:])
    an = ["entry", "scalar reads", "q rotated + first trip landed", "chunk done", "record published", "ticket drawn",
          "merge done (last of head)", "output stored (last of head)"]
    pn = ["entry", "weights requested", "weights landed (wave 0)", "flag seen", "dot products done", "output stored"]
    print("fused attention + o projection, %d attention + %d projection workgroups; us since the first workgroup entered (mean / min / max)" % (A, R))
    for title, sl, names in (("attention workgroups", slice(0, A), an), ("projection workgroups", slice(A, A + R), pn)):
        print(title + ":")
        for i, n in enumerate(names):
            col = allr[:, sl, i]
            col = col[~col.isnan()]
            if col.numel():
                print("  %-34s mean %6.2f   min %6.2f   max %6.2f   (n=%d)" % (n, col.mean(), col.min(), col.max(), col.numel()))
    print("launch span (first entry -> last projection output stored): %.2f us" %
          torch.nan_to_num(allr[:, A:, 5], nan=0.0).amax(1).mean())
    sys.exit(0)

if args.stamps:
    import ctypes
    from eetq_amd import _lib
    lib = _lib.lib()
    splits = lib.eetq_decode_attention_splits(B, H, S)
    if args.splits.split(',')[0].isdigit():
        splits = int(args.splits.split(',')[0])
    nwg = B * H * splits
    buf = torch.zeros(nwg * 8, dtype=torch.int64, device=dev)
    names = ["entry", "scalar reads", "q rotated + first trip landed", "chunk done", "record published", "ticket drawn",
             "merge done (last of head)", "output stored (last of head)"]
    rows = []
    # the stamped launch is the LAST of a graph-replayed chain of L launches (one per cache): warm clocks, warm TLBs, the
    # previous launch's tail in front of it -- the conditions the chain timing below measures (every launch of the graph
    # writes the same stamp rows; the last one's survive)
    lib.eetq_diag_attn_stamps(ctypes.c_void_p(buf.data_ptr()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(L):
            one_launch(i, splits)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(L):
                one_launch(i, splits)
    torch.cuda.current_stream().wait_stream(side)
    lib.eetq_diag_attn_stamps(None)
    for it in range(12):
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        st = buf.view(nwg, 8).cpu().double()
        t0 = st[:, 0].min()
        rel = (st - t0) / 100.0                    # microseconds since the first workgroup's entry
        rel[st == 0] = float("nan")
        rows.append(rel)
    allr = torch.stack(rows[2:])                   # [launch, workgroup, stamp]
    print("one-launch decode attention, %d workgroups (%d splits), device clock, us since the first workgroup entered" % (nwg, splits))
    print("(mean over %d launches and the workgroups that reach the stamp):" % allr.shape[0])
    for i, n in enumerate(names):
        col = allr[:, :, i]
        col = col[~col.isnan()]
        print("  %-34s mean %6.2f   min %6.2f   max %6.2f   (n=%d)" % (n, col.mean(), col.min(), col.max(), col.numel()))
    d = allr[:, :, 1:] - allr[:, :, :-1]           # per launch and workgroup: no mixing of launches
    print("phase lengths (same launch, same workgroup):")
    for i in range(7):
        col = d[:, :, i]
        col = col[~col.isnan()]
        if col.numel():
            print("  %-34s -> %-34s mean %6.2f  min %6.2f  max %6.2f us" % (names[i], names[i + 1], col.mean(), col.min(), col.max()))
    last = allr[:, :, 7]
    print("kernel span (first entry -> last output stored), mean over launches: %.2f us" % torch.nan_to_num(last, nan=0.0).amax(1).mean())
    sys.exit(0)

forms = (("one_launch", one_launch), ("two_launch", two_launch)) if args.kv_bits == 16 else (
    ("one_launch", one_launch_i8), ("two_launch", two_launch_i8))
for name, fn in forms:
    for s in args.splits.split(","):
        record(name, "tree", args.kv_bits, s, timed(fn, None if s == "default" else int(s)))
