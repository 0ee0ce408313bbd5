"""The attention entries with a per-row first key (kv_start) at Llama-2-13B heads (40 x 128), kernel launches only, timed as
tools/attn_bench.py times them: `layers` independent sets of buffers (together larger than the 256 MB Infinity Cache wherever one
set is not) stepped back to back inside one HIP graph, device events around the replays, two timed regions per figure.
usage: python tools/ragged_attn_bench.py [--rounds 2]

1. The padded entries against their twins, all starts 0 (the same process, alternating): the one-launch decode step at batch 1 and
   4 with 1 k and 16 k cached rows, the fresh 1 024-token prompt at batch 1 and 4.  Per point: the twin's two regions, the padded
   entry's two regions, the ratio of the region minima and the twin's own region spread (a ratio inside it counts as equal).
2. A ragged batch of 4 with lengths (4 096, 1 024, 256, 64), left-padded to 4 096: the decode step and the prompt pass through the
   padded entries, against the only route that batch has without them -- the twin decode entry with additive mask rows (every pad
   row streamed and thrown away), and torch's masked scaled_dot_product_attention for the prompt.
One JSON line per figure."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eetq_amd.ops as ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--cache-mb", type=int, default=512, help="bytes every chain walks through at least (2 x the Infinity Cache)")
args = ap.parse_args()
dev = "cuda:0"
H, D = 40, 128
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
    return max(2, min(24, -(-args.cache_mb * (1 << 20) // max(1, bytes_per_set))))


def compare(point, forms, L):
    """forms: [(name, fn)], the yardstick first; alternating, `rounds` regions each"""
    regions = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, fn in forms:
            regions[name].append(timed(fn, L))
    base = regions[forms[0][0]]
    out = dict(point, sets=L, yardstick=forms[0][0], yardstick_region_spread=round(max(base) / min(base), 4))
    for name, _ in forms:
        out[name + "_us"] = [round(t, 2) for t in regions[name]]
        if name != forms[0][0]:
            out[name + "_over_" + forms[0][0]] = round(min(regions[name]) / min(base), 4)
    print(json.dumps(out), flush=True)


def rope_table(rows):
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.einsum("i,j->ij", torch.arange(rows).float(), inv)
    return torch.cat([fr.cos(), fr.sin()], -1).half().to(dev)


def decode_point(B, filled, starts=None, mask_route=False):
    """the one-launch decode step on a cache of filled + 58 rows; starts None: all zero"""
    S = filled + 58
    L = sets_for(2 * B * H * S * D * 2)
    table = rope_table(S + 64)
    kc = [torch.randn(B, H, S, D, dtype=torch.float16, device=dev) for _ in range(L)]
    vc = [torch.randn(B, H, S, D, dtype=torch.float16, device=dev) for _ in range(L)]
    qkv = torch.randn(B, 1, 3 * H * D, dtype=torch.float16, device=dev)
    q, k, v = (qkv[..., i * H * D: (i + 1) * H * D].unflatten(-1, (H, D))[:, 0] for i in range(3))
    tickets = [torch.zeros(B * H + 1, dtype=torch.int32, device=dev) for _ in range(L)]
    counters = [torch.tensor(filled, dtype=torch.int64, device=dev) for _ in range(L)]
    st = torch.tensor(starts if starts is not None else [0] * B, dtype=torch.int64, device=dev)
    pos = (filled - st).contiguous()
    add = torch.zeros(B, S, dtype=torch.float16, device=dev)
    add.masked_fill_(torch.arange(S, device=dev)[None, :] < st[:, None], float("-inf"))

    def twin(i):
        return ops.rope_decode_attention(pos, q, k, v, table, kc[i], vc[i], tickets[i], slots=counters[i], kv_len=counters[i],
                                         kv_len_bias=1, mask=add if mask_route else None)

    def padded(i):
        return ops.rope_decode_attention(pos, q, k, v, table, kc[i], vc[i], tickets[i], slots=counters[i], kv_len=counters[i],
                                         kv_len_bias=1, kv_start=st)

    a, b = twin(0).float(), padded(0).float()
    point = {"what": "decode step, one launch", "batch": B, "filled": filled, "starts": starts or "zeros",
             "yardstick_route": "twin + additive mask rows" if mask_route else "twin", "max_abs_diff": round((a - b).abs().max().item(), 6)}
    compare(point, [("twin", twin), ("padded", padded)], L)


def prompt_point(B, T, starts=None):
    """a fresh prompt of T tokens; starts None: all zero against the twin, else against torch's masked attention"""
    L = sets_for(B * T * 3 * H * D * 2 + 2 * B * H * T * D * 2)
    qkv = [torch.randn(B, T, 3 * H * D, dtype=torch.float16, device=dev) for _ in range(L)]
    q = [x[..., :H * D].unflatten(-1, (H, D)) for x in qkv]
    kc = [torch.randn(B, H, T + 8, D, dtype=torch.float16, device=dev) for _ in range(L)]
    vc = [torch.randn(B, H, T + 8, D, dtype=torch.float16, device=dev) for _ in range(L)]
    st = torch.tensor(starts if starts is not None else [0] * B, dtype=torch.int64, device=dev)

    def padded(i):
        return ops.prefill_attention(q[i], kc[i], vc[i], T, kv_start=st)

    if starts is None:
        def twin(i):
            return ops.prefill_attention(q[i], kc[i], vc[i], T)
        forms, route = [("twin", twin), ("padded", padded)], "twin"
    else:
        col = torch.arange(T, device=dev)
        keep = (col[None, None, :] <= col[None, :, None]) & (col[None, None, :] >= st[:, None, None])      # [B, T, T]
        keep |= (col[None, :, None] < st[:, None, None]) & (col[None, None, :] == col[None, :, None])       # pad queries: themselves
        bias = torch.zeros(B, 1, T, T, dtype=torch.float16, device=dev).masked_fill_(~keep[:, None], float("-inf"))

        def twin(i):
            return torch.nn.functional.scaled_dot_product_attention(q[i].transpose(1, 2), kc[i][:, :, :T], vc[i][:, :, :T], attn_mask=bias)
        forms, route = [("twin", twin), ("padded", padded)], "torch scaled_dot_product_attention with a mask"
    a, b = forms[0][1](0), padded(0)
    a = a.transpose(1, 2) if starts is not None else a
    real = (torch.arange(T, device=dev)[None, :] >= st[:, None])[:, :, None, None]
    diff = ((a.float() - b.float()) * real).abs().max().item()
    point = {"what": "fresh prompt", "batch": B, "tokens": T, "starts": starts or "zeros", "yardstick_route": route,
             "max_abs_diff_real_rows": round(diff, 6)}
    compare(point, forms, L)


for B in (1, 4):
    for filled in (1024, 16384):
        decode_point(B, filled)
for B in (1, 4):
    prompt_point(B, 1024)
RAGGED = [4096 - n for n in (4096, 1024, 256, 64)]
decode_point(4, 4096, starts=RAGGED, mask_route=True)
prompt_point(4, 4096, starts=RAGGED)
