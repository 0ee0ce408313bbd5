"""The ring-cache attention entries (ring=True) at Llama-2-13B heads (40 x 128), kernel launches only, timed as
tools/window_attn_bench.py times them: independent sets of buffers (together at least 512 MB, twice the Infinity Cache) stepped
back to back inside one HIP graph, device events around the replays, the yardstick and the ring entry alternating in one process,
two timed regions per figure.  The yardstick is always the windowed entry on a static cache (window=W), whose device code is the
parent's.
usage: python tools/ring_attn_bench.py [--rounds 2]

1. The decode step (one launch) at logical length 16 384, batch 1 and 4, W = 1 024 / 4 096: the static cache has 16 384 + 58 rows,
   the ring ring_rows(W, 512).  What a rolling decoder pays or gains against the windowed decoder it replaces.
2. The same pair at EQUAL capacity: a static cache of ring_rows(W, 512) rows filled to its last row against the ring of the same
   rows at the same length (the window does not wrap) and at length 16 384 (it does).  Chunk count and LONG form are equal here, so
   the difference is the wrap arithmetic and the explicit validity select.
3. A 512-row prompt piece behind 4 096 rows with W = 1 024: static cache of 4 608 + 8 rows against the ring of ring_rows(1 024, 512).
One JSON line per figure; every ratio carries the twin's own region spread (a ratio inside it counts as equal)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eetq_amd.ops as ops  # noqa: E402
from eetq_amd.utils.kv_cache import ring_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--cache-mb", type=int, default=512, help="bytes every chain walks through at least (2 x the Infinity Cache)")
args = ap.parse_args()
dev = "cuda:0"
H, D = 40, 128
LOGICAL = 16384
torch.manual_seed(0)


def timed(fn, L, min_ms=30.0):
    """microseconds per call of fn(i), i over L buffer sets, one graph of L calls; replays until min_ms have been timed"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(L):
            fn(i)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(L):
                fn(i)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 4
    while True:
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_ms or reps >= 4096:
            return ms * 1e3 / (reps * L)
        reps *= 4


def sets_for(bytes_per_set):
    return max(2, min(48, -(-args.cache_mb * (1 << 20) // max(1, bytes_per_set))))


def compare(point, forms):
    """forms: [(name, fn, sets)], the yardstick first; alternating, `rounds` regions each"""
    regions = {name: [] for name, _, _ in forms}
    for _ in range(args.rounds):
        for name, fn, L in forms:
            regions[name].append(timed(fn, L))
    base = regions[forms[0][0]]
    out = dict(point, yardstick=forms[0][0], yardstick_region_spread=round(max(base) / min(base), 4))
    for name, _, L in forms:
        out[name + "_sets"] = L
        out[name + "_us"] = [round(t, 2) for t in regions[name]]
        if name != forms[0][0]:
            out[name + "_over_" + forms[0][0]] = round(min(regions[name]) / min(base), 4)
    print(json.dumps(out), flush=True)


def rope_table(rows):
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.einsum("i,j->ij", torch.arange(rows).float(), inv)
    return torch.cat([fr.cos(), fr.sin()], -1).half().to(dev)


TABLE = rope_table(LOGICAL + 64)


def decode_form(B, rows, n, W, ring):
    """the one-launch decode step of the token at logical row n on caches of `rows` rows -> (fn, sets)"""
    L = sets_for(2 * B * H * rows * D * 2)
    kc = [torch.randn(B, H, rows, D, dtype=torch.float16, device=dev) for _ in range(L)]
    vc = [torch.randn(B, H, rows, D, dtype=torch.float16, device=dev) for _ in range(L)]
    qkv = torch.randn(B, 1, 3 * H * D, dtype=torch.float16, device=dev)
    q, k, v = (qkv[..., i * H * D: (i + 1) * H * D].unflatten(-1, (H, D))[:, 0] for i in range(3))
    tickets = [torch.zeros(B * H + 1, dtype=torch.int32, device=dev) for _ in range(L)]
    counters = [torch.tensor(n, dtype=torch.int64, device=dev) for _ in range(L)]
    pos = torch.full((B,), n, dtype=torch.int64, device=dev)
    kw = {"ring": True} if ring else {}
    return (lambda i: ops.rope_decode_attention(pos, q, k, v, TABLE, kc[i], vc[i], tickets[i], slots=counters[i], kv_len=counters[i],
                                                kv_len_bias=1, window=W, **kw)), L


def decode_points(B, W):
    R = ring_rows(W, 512)
    point = {"what": "decode step, one launch", "batch": B, "window": W, "ring_rows": R}
    # 1. the decoder's view: a 16 k-row static cache against the ring
    compare(dict(point, logical_length=LOGICAL, static_rows=LOGICAL + 58),
            [("window_static",) + decode_form(B, LOGICAL + 58, LOGICAL - 1, W, False), ("ring",) + decode_form(B, R, LOGICAL - 1, W, True)])
    torch.cuda.empty_cache()
    # 2. equal capacity
    compare(dict(point, static_rows=R, pair="equal capacity"),
            [("window_static",) + decode_form(B, R, R - 1, W, False), ("ring_unwrapped",) + decode_form(B, R, R - 1, W, True),
             ("ring_wrapped",) + decode_form(B, R, LOGICAL - 1, W, True)])
    torch.cuda.empty_cache()


def prompt_point(B, T, behind, W):
    keys, R = behind + T, ring_rows(W, T)
    n = torch.tensor([keys], dtype=torch.int64, device=dev)

    def form(rows, bound, ring):
        L = sets_for(B * T * 3 * H * D * 2 + 2 * B * H * rows * D * 2)
        qkv = [torch.randn(B, T, 3 * H * D, dtype=torch.float16, device=dev) for _ in range(L)]
        q = [x[..., :H * D].unflatten(-1, (H, D)) for x in qkv]
        kc = [torch.randn(B, H, rows, D, dtype=torch.float16, device=dev) for _ in range(L)]
        vc = [torch.randn(B, H, rows, D, dtype=torch.float16, device=dev) for _ in range(L)]
        kw = {"ring": True} if ring else {}
        return (lambda i: ops.prefill_attention(q[i], kc[i], vc[i], bound, kv_len=n, window=W, **kw)), L

    point = {"what": "appended prompt piece", "batch": B, "tokens": T, "behind": behind, "window": W, "ring_rows": R,
             "static_rows": keys + 8, "splits_rule": ops.prefill_attention_splits(B, H, T, min(keys + 8, W + min(T, 128)))}
    compare(point, [("window_static",) + form(keys + 8, keys + 8, False), ("ring",) + form(R, 1 << 30, True)])


for B in (1, 4):
    for W in (1024, 4096):
        decode_points(B, W)
prompt_point(1, 512, 4096, 1024)
