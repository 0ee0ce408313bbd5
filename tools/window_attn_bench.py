"""The sliding-window attention entries (window=W) at Llama-2-13B heads (40 x 128), kernel launches only, timed as
tools/ragged_attn_bench.py times them: `sets` independent sets of buffers (together at least 512 MB, twice the Infinity Cache)
stepped back to back inside one HIP graph, device events around the replays, the yardstick and the windowed entry alternating in
one process, two timed regions per figure.
usage: python tools/window_attn_bench.py [--rounds 2]

1. Cost of the opt-in: W >= keys against the plain twin of the same build (the twin's code is unchanged).  The one-launch decode step
   at batch 1 and 4 with 1 k and 16 k cached rows, the fresh 1 024-token prompt.  Per point: both entries' regions, the ratio of the
   region minima and the twin's own region spread (a ratio inside it counts as equal).
2. Gain: the decode step with 16 384 cached rows and W = 4 096 / 1 024, against the plain step at 16 384 rows and at W rows (equal
   attended rows); the fresh prompt of 8 192 tokens with W = 1 024 against the plain prompt.
3. Appended prompts: 16 rows behind 4 096 cached ones with W = 1 024 -- what the (untuned) split rule picks, against one share and
   against the plain appended prompt under its own rule.
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


def decode_point(B, filled, windows, short=()):
    """the one-launch decode step on a cache of filled + 58 rows: the plain twin, window=W for every W, and the plain twin with
    only `n` rows filled for every n of `short` (the same buffers, a smaller counter: equal attended rows)"""
    S = filled + 58
    L = sets_for(2 * B * H * S * D * 2)
    table = rope_table(S + 64)
    kc = [torch.randn(B, H, S, D, dtype=torch.float16, device=dev) for _ in range(L)]
    vc = [torch.randn(B, H, S, D, dtype=torch.float16, device=dev) for _ in range(L)]
    qkv = torch.randn(B, 1, 3 * H * D, dtype=torch.float16, device=dev)
    q, k, v = (qkv[..., i * H * D: (i + 1) * H * D].unflatten(-1, (H, D))[:, 0] for i in range(3))
    tickets = [torch.zeros(B * H + 1, dtype=torch.int32, device=dev) for _ in range(L)]

    def step(n, **kw):
        counters = [torch.tensor(n, dtype=torch.int64, device=dev) for _ in range(L)]
        pos = torch.full((B,), n, dtype=torch.int64, device=dev)
        return lambda i: ops.rope_decode_attention(pos, q, k, v, table, kc[i], vc[i], tickets[i], slots=counters[i], kv_len=counters[i],
                                                   kv_len_bias=1, **kw)

    forms = [("twin", step(filled))]
    forms += [("window_%d" % W, step(filled, window=W)) for W in windows]
    forms += [("twin_at_%d_rows" % n, step(n - 1)) for n in short]
    point = {"what": "decode step, one launch", "batch": B, "filled": filled, "capacity": S}
    wide = [W for W in windows if W > filled]
    if wide:
        point["wide_window_bits_equal_twin"] = bool(torch.equal(forms[0][1](0), step(filled, window=wide[0])(0)))
    compare(point, forms, L)


def prompt_point(B, T, windows):
    """a fresh prompt of T tokens: the plain twin and window=W"""
    L = sets_for(B * T * 3 * H * D * 2 + 2 * B * H * T * D * 2)
    qkv = [torch.randn(B, T, 3 * H * D, dtype=torch.float16, device=dev) for _ in range(L)]
    q = [x[..., :H * D].unflatten(-1, (H, D)) for x in qkv]
    kc = [torch.randn(B, H, T + 8, D, dtype=torch.float16, device=dev) for _ in range(L)]
    vc = [torch.randn(B, H, T + 8, D, dtype=torch.float16, device=dev) for _ in range(L)]
    forms = [("twin", lambda i: ops.prefill_attention(q[i], kc[i], vc[i], T))]
    for W in windows:
        forms.append(("window_%d" % W, lambda i, W=W: ops.prefill_attention(q[i], kc[i], vc[i], T, window=W)))
    point = {"what": "fresh prompt", "batch": B, "tokens": T}
    wide = [W for W in windows if W >= T]
    if wide:
        point["wide_window_bits_equal_twin"] = bool(torch.equal(forms[0][1](0), ops.prefill_attention(q[0], kc[0], vc[0], T, window=wide[0])))
    compare(point, forms, L)


def append_point(B, T, behind, W):
    """T rows behind `behind` cached ones through the device length: the plain entry under its rule, window=W under the windowed rule
    and with one share"""
    keys = behind + T
    L = sets_for(B * T * 3 * H * D * 2 + 2 * B * H * keys * D * 2)
    qkv = [torch.randn(B, T, 3 * H * D, dtype=torch.float16, device=dev) for _ in range(L)]
    q = [x[..., :H * D].unflatten(-1, (H, D)) for x in qkv]
    kc = [torch.randn(B, H, keys + 8, D, dtype=torch.float16, device=dev) for _ in range(L)]
    vc = [torch.randn(B, H, keys + 8, D, dtype=torch.float16, device=dev) for _ in range(L)]
    n = torch.tensor([keys], dtype=torch.int64, device=dev)
    rule_plain = ops.prefill_attention_splits(B, H, T, keys + 8)
    rule_win = ops.prefill_attention_splits(B, H, T, min(keys + 8, W + min(T, 128)))
    forms = [("twin", lambda i: ops.prefill_attention(q[i], kc[i], vc[i], keys + 8, kv_len=n)),
             ("window_rule", lambda i: ops.prefill_attention(q[i], kc[i], vc[i], keys + 8, kv_len=n, window=W)),
             ("window_one_share", lambda i: ops.prefill_attention(q[i], kc[i], vc[i], keys + 8, kv_len=n, window=W, splits=1))]
    point = {"what": "appended prompt", "batch": B, "tokens": T, "behind": behind, "window": W, "twin_splits": rule_plain,
             "window_rule_splits": rule_win}
    compare(point, forms, L)


# 1. the cost of the opt-in: a window over everything against the plain twin
for B in (1, 4):
    for filled in (1024, 16384):
        decode_point(B, filled, windows=(1 << 20,))
prompt_point(1, 1024, windows=(1 << 20,))
# 2. the gain
for B in (1, 4):
    decode_point(B, 16384, windows=(4096, 1024), short=(4096, 1024))
prompt_point(1, 8192, windows=(1024,))
# 3. appended prompts and the untuned split rule
append_point(1, 16, 4096, 1024)
