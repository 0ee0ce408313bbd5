"""One verify step of GraphDecoder(speculative=k) against one plain step of the same decoder, graph-replayed, and the tokens/s
at the two bounds of the acceptance (every draft token right / none), at the Llama-2-13B shapes of bench.py's config 5, batch 1.

The model is config 5's random initialisation with two changes that make its greedy continuation KNOWN without changing what the
kernels stream: the output and down projections are scaled by 2^-10 before quantisation (their int8 codes keep the full range,
the scales shrink), so the hidden state stays within a hair of the token's embedding, and row perm[t] of lm_head is the
embedding of t for one vocabulary-wide cycle perm: the greedy token after t is perm[t].  The ``draft=`` hook then serves
perm[t], perm[perm[t]], ... (all accepted) or those + 1 (all rejected), switched by a static device flag, so ONE captured verify
graph serves both bounds.

Per (cache rows, k): microseconds of one replay of the plain one-step graph, of the plain 7-step graph per token, of the verify
graph at either bound (median of --reps timings of --chain consecutive replays), tokens/s = tokens handed over / time, and the
break-even: the tokens per verify step at which speculative decoding equals the plain 7-step graph, verify / plain-per-token.
Writes the table to --out (default profiles/spec_decode.txt).
--spec-attention prompt,rows: the verify step's attention (GraphDecoder(spec_attention=...)), one table row per value, "rows" next to
"prompt" on the same model in the same session (profiles/spec_decode_rows.txt).
--kv-bits 8: the decoder on an int8 KV cache (GraphDecoder(kv_bits=8, kv8_append=True)): plain steps and verify steps both run on
int8 rows, so verify / plain is in plain INT8 steps (profiles/spec_decode_kv8.txt).
usage: python tools/spec_bench.py [--caches 1024,4096] [--ks 2,4,8] [--chain 16] [--reps 7] [--layers 40] [--spec-attention prompt]
                                  [--kv-bits 16]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--caches", default="1024,4096")
ap.add_argument("--ks", default="2,4,8")
ap.add_argument("--chain", type=int, default=16, help="consecutive replays per timing (a multiple of 7 is not needed)")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--layers", type=int, default=40, help="decoder layers (40 = Llama-2-13B; fewer for a quick look)")
ap.add_argument("--spec-attention", default="prompt", help="comma-separated: prompt (the MFMA prompt kernel), rows (the few-row kernel)")
ap.add_argument("--kv-bits", type=int, default=16, choices=(16, 8), help="8: an int8 KV cache (kv8_append=True)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_decode.txt"))
args = ap.parse_args()
DEV = "cuda:0"
VOCAB = 32000


def build_model():
    import transformers
    from eetq_amd.utils import eet_accelerator
    cfg = transformers.LlamaConfig(hidden_size=5120, intermediate_size=13824, num_hidden_layers=args.layers, num_attention_heads=40,
                                   num_key_value_heads=40, vocab_size=VOCAB, max_position_embeddings=8192)
    torch.manual_seed(0)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device(DEV):
            model = transformers.LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(old)
    order = torch.randperm(VOCAB, generator=torch.Generator().manual_seed(2))
    perm = torch.empty(VOCAB, dtype=torch.long)
    perm[order] = order.roll(-1)                       # one cycle through the whole vocabulary
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(VOCAB)
    with torch.no_grad():
        for layer in model.model.layers:
            layer.self_attn.o_proj.weight.mul_(2.0 ** -10)
            layer.mlp.down_proj.weight.mul_(2.0 ** -10)
        model.lm_head.weight.copy_(model.model.embed_tokens.weight[inv.to(DEV)])
    eet_accelerator(model, quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)
    return model, perm.to(DEV)


def timed(replay, prepare):
    """median microseconds of one replay: args.reps timings of args.chain consecutive replays, each after prepare()"""
    us = []
    for _ in range(args.reps + 1):
        prepare()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.chain):
            replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / args.chain)
    return statistics.median(us[1:])                   # (the first timing warms up)


def main():
    from eetq_amd.utils import GraphDecoder
    model, perm = build_model()
    cache_kw = {"kv_bits": 8, "kv8_append": True} if args.kv_bits == 8 else {}
    lines = ["# tools/spec_bench.py: Llama-2-13B shapes (%d layers, random init, W8A16%s), batch 1, %s"
             % (args.layers, ", int8 KV cache" if args.kv_bits == 8 else "", torch.cuda.get_device_name(0)),
             "# us per graph replay (median of %d timings of %d consecutive replays); tokens/s = tokens handed over / time" % (args.reps, args.chain),
             "# break-even = verify_us / plain7_us_per_token: tokens per verify step at which the speculative decoder equals the plain one",
             "%6s %3s %6s %10s %12s %10s %11s %10s %10s %10s %10s" % ("cache", "k", "attn", "plain1_us", "plain7_us/t", "verify_us", "verify/pl1",
                                                                    "tok/s_pl7", "tok/s_all", "tok/s_none", "break-even")]
    print("\n".join(lines), flush=True)
    mode = torch.zeros(1, dtype=torch.long, device=DEV)          # 0: the right tokens, 1: wrong ones

    for cache in [int(c) for c in args.caches.split(",")]:
        prompt = torch.randint(0, VOCAB, (1, cache - 1), generator=torch.Generator().manual_seed(1)).to(DEV)
        for k, attn in [(int(x), a) for x in args.ks.split(",") for a in args.spec_attention.split(",")]:
            def draft(dec):
                toks, t = [], dec.s_tok
                for _ in range(dec.speculative):
                    t = perm[t]
                    toks.append(t)
                return (torch.cat(toks, dim=1) + mode) % VOCAB

            span = args.chain * max(k + 1, 7) + k + 4              # rows one timing may write behind the prompt
            max_len = cache + span + 8
            with torch.no_grad():
                dec = GraphDecoder(model, 1, max_len, speculative=k, draft=draft, spec_attention=attn, **cache_kw)

                dec.generate(prompt, 1)                             # the prompt pass and one token: `cache` rows cached or pending
                first = dec.s_tok.clone()
                counters = [layer.cumulative_length for layer in dec.cache.layers]

                def prepare():
                    # back to the state behind the prompt (its cache rows are never overwritten), with an unbounded limit
                    dec.s_pos.fill_(cache - 1)
                    dec.s_idx.fill_(1)
                    dec.s_tok.copy_(first)
                    for c in counters:
                        c.fill_(cache - 1)
                    dec.s_limit.fill_(1 << 40)
                    dec.s_stats.zero_()

                assert cache + args.chain * (k + 1) + k <= max_len and cache + args.chain * 7 <= max_len   # every row written lies inside the cache
                plain1 = timed(dec.graph.replay, prepare)
                plain7 = timed(dec.graph_n.replay, prepare) / dec.steps_per_graph
                mode.fill_(0)
                v_all = timed(dec.graph_spec.replay, prepare)
                steps, tokens = dec.spec_stats()
                per_all = tokens / max(steps, 1)
                mode.fill_(1)
                v_none = timed(dec.graph_spec.replay, prepare)
                steps, tokens = dec.spec_stats()
                per_none = tokens / max(steps, 1)
            verify = (v_all + v_none) / 2
            line = "%6d %3d %6s %10.1f %12.1f %10.1f %11.3f %10.1f %10.1f %10.1f %10.2f" % (
                cache, k, attn, plain1, plain7, verify, verify / plain1, 1e6 / plain7, 1e6 * per_all / v_all, 1e6 * per_none / v_none, verify / plain7)
            print(line, flush=True)
            lines.append(line)
            note = "#        verify_us / tokens per step as counted on the device: right drafts %.1f / %.2f, wrong drafts %.1f / %.2f" % (
                v_all, per_all, v_none, per_none)
            print(note, flush=True)
            lines.append(note)
            del dec
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
