"""One 13B-shaped decoder layer (hidden 5120, 40 heads x 128, W8A16) running a 64-token prompt behind 2 048 cached rows of a static
cache: wall time per call of the model forward, under ``appended_static_prefill`` (the library's prompt kernel with the cache's
device counter as its length) and without the promise (the stock attention call over all pre-allocated rows under the model's
mask).  --tree DIR imports the package from DIR, the built tree of another commit (without the promise where it has none).
usage: python tools/append_layer_bench.py [--tree DIR]"""
import contextlib, sys, os, time
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(TREE))
import torch, transformers
from eetq_amd.utils import eet_accelerator
import eetq_amd.modules.llama_modules as lm
CACHED, T, ROWS = 2048, 64, 2048 + 64 + 8
cfg = transformers.LlamaConfig(hidden_size=5120, intermediate_size=13824, num_hidden_layers=1, num_attention_heads=40,
                               num_key_value_heads=40, vocab_size=32000, max_position_embeddings=4096)
torch.manual_seed(0); torch.set_default_dtype(torch.float16)
with torch.device("cuda:0"):
    model = transformers.LlamaForCausalLM(cfg).eval()
torch.set_default_dtype(torch.float32)
eet_accelerator(model, quantize=True, fused_attn=True, fused_mlp=True, fused_norm=True, fused_residual=True)
g = torch.Generator().manual_seed(1)
first, more = torch.randint(0, 32000, (1, CACHED), generator=g).cuda(), torch.randint(0, 32000, (1, T), generator=g).cuda()
cache = transformers.StaticCache(config=cfg, max_cache_len=ROWS)
pos = torch.arange(CACHED, CACHED + T, device="cuda:0")


def timed(ctx, n=30):
    def call():
        cache.layers[0].cumulative_length.fill_(CACHED)          # the same 64 rows behind the same 2 048 every time
        with ctx():
            return model.model(more, past_key_values=cache, cache_position=pos, use_cache=True).last_hidden_state
    for _ in range(5):
        out = call()
    best = 1e30
    for _ in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n):
            call()
        torch.cuda.synchronize(); best = min(best, (time.perf_counter() - t0) / n * 1e6)
    return best, out


with torch.no_grad():
    model.model(first[:, :1], past_key_values=cache, use_cache=True)
    cache.reset()
    model.model(first, past_key_values=cache, cache_position=torch.arange(CACHED, device="cuda:0"), use_cache=True)
    print("tree %s" % os.path.abspath(TREE))
    stock, a = timed(contextlib.nullcontext)
    print("64 rows behind 2048, 1 layer, no promise (stock attention call): %.1f us per forward" % stock)
    if hasattr(lm, "appended_static_prefill"):
        fast, b = timed(lm.appended_static_prefill)
        print("64 rows behind 2048, 1 layer, appended_static_prefill:           %.1f us per forward" % fast)
        print("max |difference| of the layer output %.4g (|output| max %.4g)" % ((a.float() - b.float()).abs().max().item(), a.float().abs().max().item()))
