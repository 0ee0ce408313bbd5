"""Prompt attention (eetq_prefill_attention_f16) against a float32 softmax(q k^T) v of the same inputs (max abs error per case) and,
chain-timed, against torch's scaled_dot_product_attention at Llama-2-13B shapes (40 heads x 128, 1 024 tokens), batch 1 and 4.
usage: python tools/prefill_attn_bench.py
       python tools/prefill_attn_bench.py --append [--baseline] [--tree DIR]
--append: prompts appended behind cached rows (eetq_prefill_attention_dev_f16) at 13B head geometry (40 x 128) and one grouped
geometry (32 / 8 x 128): Tq 16 .. 512 behind 512 .. 4096 rows, batch 1 and 4; per shape the chain time of the host-length unsplit
call, the device-length unsplit call and forced splits 2 .. 16, the rule's choice, and the largest max abs error of those calls
against the float32 reference; then the fresh 1 024-token shapes with the host and the device length.  --baseline: the host-length
unsplit call only (every build has it).  --tree DIR: import the package from DIR, the built tree of another commit, so that its
`ops.prefill_attention(q, k, v, keys)` is timed in the same session, alternating with this one.
--append --kv-bits 8: the int8-row form (eetq_prefill_attention_i8kv_f16) against the fp16 appended form at the same shapes: Tq 16,
128 and 512 behind 1 024, 4 096 and 16 384 rows, batch 1 and 4; per shape the fp16 device-length unsplit call and the fp16 call at
the rule's count, then the int8 unsplit call, forced splits 2 .. 16 and the rule's count (the same rule), and at batch 1 the
largest error of the int8 calls against a float32 reference over the dequantised rows."""
import sys, os, torch
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(TREE))
sys.path.insert(0, os.path.join(os.path.abspath(TREE), "tools"))
import eetq_amd.ops as ops
from sweep import chain_us
dev = "cuda:0"
torch.manual_seed(0)


def reference(q, kc, vc, keys, base):
    B, T, H, D = q.shape
    Hkv = kc.shape[1]
    k, v = kc[:, :, :keys].float(), vc[:, :, :keys].float()
    if Hkv != H:
        k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    sc = torch.matmul(q.transpose(1, 2).float(), k.transpose(2, 3)) / D ** 0.5
    mask = torch.arange(keys, device=dev)[None, :] > (torch.arange(T, device=dev)[:, None] + base)
    return torch.matmul(torch.softmax(sc.masked_fill(mask, float("-inf")), -1), v).transpose(1, 2)


def append_table(baseline):
    D, pad = 128, 8
    print("tree %s%s" % (os.path.abspath(TREE), " (baseline: host length, unsplit)" if baseline else ""))
    print("H/Hkv B Tq cached | host dev s2 s4 s8 s16 [us] | rule | max abs err")
    shapes = [(H, Hkv, B, T, base) for H, Hkv in ((40, 40), (32, 8)) for B in (1, 4) for base in (512, 2048, 4096) for T in (16, 64, 128, 512)]
    shapes += [(40, 40, B, 1024, 0) for B in (1, 4)]                      # the fresh prompt of the flagship workload
    for H, Hkv, B, T, base in shapes:
        keys = base + T
        qkv = torch.randn(B, T, (H + 2 * Hkv) * D, dtype=torch.float16, device=dev)
        q = qkv[..., :H * D].unflatten(-1, (H, D))
        kc = torch.randn(B, Hkv, keys + pad, D, dtype=torch.float16, device=dev)
        vc = torch.randn(B, Hkv, keys + pad, D, dtype=torch.float16, device=dev)
        times, err, rule = [chain_us(lambda i: ops.prefill_attention(q, kc, vc, keys), 10)], float("nan"), "-"
        if not baseline:
            n = torch.tensor([keys], dtype=torch.int64, device=dev)
            ref = reference(q, kc, vc, keys, base)
            err = (ops.prefill_attention(q, kc, vc, keys).float() - ref).abs().max().item()
            err = max(err, (ops.prefill_attention(q, kc, vc, keys + pad, kv_len=n, splits=1).float() - ref).abs().max().item())
            times.append(chain_us(lambda i: ops.prefill_attention(q, kc, vc, keys + pad, kv_len=n, splits=1), 10))
            for ns in (2, 4, 8, 16):
                ws = torch.empty(B * H * T * ns * (D + 2), dtype=torch.float32, device=dev)
                err = max(err, (ops.prefill_attention(q, kc, vc, keys + pad, kv_len=n, splits=ns, workspace=ws).float() - ref).abs().max().item())
                times.append(chain_us(lambda i: ops.prefill_attention(q, kc, vc, keys + pad, kv_len=n, splits=ns, workspace=ws), 10))
            rule = "%d" % ops.prefill_attention_splits(B, H, T, keys + pad)
            del ref
        print("%d/%d %d %d %d | %s | %s | %.5f" % (H, Hkv, B, T, base, " ".join("%.1f" % t for t in times), rule, err), flush=True)


def quantize_rows(x):
    """the row quantiser of include/eetq_amd.h on the GPU: int8 [..., D], fp16 scale [...]"""
    s = (x.float().abs().amax(-1) * (1.0 / 127.0)).half()
    r = x.float() / s.float()[..., None]
    r = torch.where(s[..., None] == 0, torch.zeros_like(r), r)
    q = (torch.sign(r) * torch.floor(r.abs() + 0.5)).clamp(-127, 127).to(torch.int8)
    return q, s


def append_table_kv8():
    D, pad = 128, 8
    print("tree %s (int8 rows against fp16 rows)" % os.path.abspath(TREE))
    print("H/Hkv B Tq cached | fp16: dev rule-split | int8: dev s2 s4 s8 s16 rule-split [us] | rule | max abs err (int8, B = 1)")
    shapes = [(H, Hkv, B, T, base) for H, Hkv in ((40, 40), (32, 8)) for B in (1, 4) for base in (1024, 4096, 16384) for T in (16, 128, 512)]
    for H, Hkv, B, T, base in shapes:
        keys = base + T
        qkv = torch.randn(B, T, (H + 2 * Hkv) * D, dtype=torch.float16, device=dev)
        q = qkv[..., :H * D].unflatten(-1, (H, D))
        kc = torch.randn(B, Hkv, keys + pad, D, dtype=torch.float16, device=dev)
        vc = torch.randn(B, Hkv, keys + pad, D, dtype=torch.float16, device=dev)
        k8, ks = quantize_rows(kc)
        v8, vs = quantize_rows(vc)
        sc = torch.stack([ks, vs], dim=-1).contiguous()
        n = torch.tensor([keys], dtype=torch.int64, device=dev)
        rule = ops.prefill_attention_splits(B, H, T, keys + pad)
        ws = {ns: torch.empty(max(1, B * H * T * ns * (D + 2)), dtype=torch.float32, device=dev) for ns in (2, 4, 8, 16)}
        ws[1] = None
        f16 = [chain_us(lambda i: ops.prefill_attention(q, kc, vc, keys + pad, kv_len=n, splits=ns, workspace=ws[ns]), 10) for ns in (1, rule)]
        i8 = [chain_us(lambda i: ops.prefill_attention_i8kv(q, k8, v8, sc, keys + pad, kv_len=n, splits=ns, workspace=ws[ns]), 10)
              for ns in (1, 2, 4, 8, 16, rule)]
        err = float("nan")
        if B == 1:
            ref = reference(q, k8.float() * ks.float()[..., None], v8.float() * vs.float()[..., None], keys, base)
            err = max((ops.prefill_attention_i8kv(q, k8, v8, sc, keys + pad, kv_len=n, splits=ns, workspace=ws[ns]).float() - ref).abs().max().item()
                      for ns in (1, 2, 4, 8, 16))
            del ref
        print("%d/%d %d %d %d | %s | %s | %d | %.5f" % (H, Hkv, B, T, base, " ".join("%.1f" % t for t in f16), " ".join("%.1f" % t for t in i8),
                                                        rule, err), flush=True)


if "--append" in sys.argv:
    if "--kv-bits" in sys.argv and sys.argv[sys.argv.index("--kv-bits") + 1] == "8":
        append_table_kv8()
    else:
        append_table("--baseline" in sys.argv)
    sys.exit(0)
def run(B, T, H, Hkv, S, D=128, base=0):
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, dtype=torch.float16, device=dev)
    q = qkv[..., :H * D].unflatten(-1, (H, D))
    kc = torch.randn(B, Hkv, S, D, dtype=torch.float16, device=dev)
    vc = torch.randn(B, Hkv, S, D, dtype=torch.float16, device=dev)
    keys = base + T
    out = ops.prefill_attention(q, kc, vc, keys)
    qq = q.transpose(1, 2).float()
    k, v = kc[:, :, :keys].float(), vc[:, :, :keys].float()
    if Hkv != H:
        k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
    sc = torch.matmul(qq, k.transpose(2, 3)) / D ** 0.5
    mask = torch.arange(keys, device=dev)[None, :] > (torch.arange(T, device=dev)[:, None] + base)
    sc = sc.masked_fill(mask, float("-inf"))
    ref = torch.matmul(torch.softmax(sc, -1), v).transpose(1, 2)
    err = (out.float() - ref).abs().max().item()
    print("B %d T %d H %d Hkv %d S %d base %d: max abs err %.5f (ref max %.3f) nan %s" % (B, T, H, Hkv, S, base, err, ref.abs().max().item(), bool(out.isnan().any())), flush=True)
    return q, kc, vc, keys
run(1, 128, 2, 2, 160)
run(1, 200, 4, 2, 256)
run(2, 130, 4, 4, 300, base=37)
run(1, 64, 2, 1, 64)
q, kc, vc, keys = run(1, 1024, 40, 40, 1082)
def f(i): return ops.prefill_attention(q, kc, vc, keys)
print("B1 T1024 H40: %.1f us" % chain_us(f, 10))
qt = q.transpose(1, 2)
def g(i): return torch.nn.functional.scaled_dot_product_attention(qt, kc[:, :, :keys], vc[:, :, :keys], is_causal=True)
print("torch sdpa:   %.1f us" % chain_us(g, 10))
q, kc, vc, keys = run(4, 1024, 40, 40, 1082)
print("B4 T1024 H40: %.1f us" % chain_us(f, 10))
