"""One call of every instantiation of the decode-attention kernels (eetq_amd/csrc/attn_decode.hip) through the C entries, on seeded
inputs, one line per call:

    entry D mask length sha256(everything the call produces)

"Everything" is the output, and in the one-launch form also both caches whole (the written row, and any row that should not have
been), the scale tensor of an int8 cache, the tickets and the advanced counter; a call the entry refuses prints its status
instead.  Covered: {fp16, int8} x {two-launch, one-launch} x D {64, 128} x mask {none, rows with -inf} x {short, LONG}, the 16
fp16 forms with a per-row first key (PAD), and one dropped step (a slot outside the cache) per format together with
eetq_decode_dropped_steps.  Two batch rows, 4 heads on 2 kv heads, fewer filled rows than the cache holds; short = 96 rows in 2
chunks, LONG = one chunk of more than 16 blocks (320 rows at D = 128, 576 at D = 64).  Two builds of the library that print the same
lines compute the same bits in every instantiation.  Needs an MI355X.

    python tools/attn_entry_digest.py [--lib OTHER/libeetq_amd.so] > digest.txt
"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
B, H, HKV = 2, 4, 2
ENTRIES = ("eetq_decode_attention_f16", "eetq_decode_attention_padded_f16", "eetq_decode_attention_i8kv_f16",
           "eetq_rope_decode_attention_bounded_f16", "eetq_rope_decode_attention_padded_f16",
           "eetq_rope_decode_attention_i8kv_f16", "eetq_decode_dropped_steps")


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _longs(*v):
    return (ctypes.c_long * len(v))(*v)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libeetq_amd.so to call instead of the package's")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/attn_entry_digest.py needs a GPU"
    from eetq_amd import _lib
    L = _lib.lib()
    if args.lib:
        other = ctypes.CDLL(os.path.abspath(args.lib))
        for name in ENTRIES:
            getattr(other, name).argtypes = getattr(L, name).argtypes
            getattr(other, name).restype = getattr(L, name).restype
        L = other
    g = torch.Generator().manual_seed(41)
    dropped = ctypes.c_ulonglong(0)
    assert L.eetq_decode_dropped_steps(ctypes.byref(dropped), 1) == 0

    def case(fmt, form, D, masked, S, splits, pad=False, drop=False):
        filled = S - 9
        q = (torch.rand(B, H, D, generator=g) - 0.5).half().to(DEV)
        knew = (torch.rand(B, HKV, D, generator=g) - 0.5).half().to(DEV)
        vnew = (torch.rand(B, HKV, D, generator=g) - 0.5).half().to(DEV)
        if fmt == "f16":
            kc = (torch.rand(B, HKV, S, D, generator=g) - 0.5).half().to(DEV)
            vc = (torch.rand(B, HKV, S, D, generator=g) - 0.5).half().to(DEV)
            scales = None
        else:
            kc = torch.randint(-127, 128, (B, HKV, S, D), dtype=torch.int8, generator=g).to(DEV)
            vc = torch.randint(-127, 128, (B, HKV, S, D), dtype=torch.int8, generator=g).to(DEV)
            scales = (torch.rand(B, HKV, S, 2, generator=g) * 4e-3 + 1e-4).half().to(DEV)
        mask = None
        if masked:
            mask = (torch.rand(B, S, generator=g) - 0.5).half()
            mask[torch.rand(B, S, generator=g) < 0.2] = float("-inf")
            mask[:, filled - 1] = 0.0   # no row of the batch is masked out whole
            mask = mask.to(DEV)
        theta = torch.rand(S, D // 2, generator=g) * 6.0
        cos_sin = torch.cat([theta.cos(), theta.sin()], dim=1).half().to(DEV)
        kv_len = torch.tensor([filled], dtype=torch.int64, device=DEV)
        counter = torch.tensor([5], dtype=torch.int64, device=DEV)
        kv_start = torch.tensor([3, 40], dtype=torch.int64, device=DEV)
        positions = torch.tensor([filled, filled - 3], dtype=torch.int64, device=DEV)
        slots = torch.tensor([filled, S if drop else filled], dtype=torch.int64, device=DEV)
        tickets = torch.zeros(B * H + 1, dtype=torch.int32, device=DEV)
        out = torch.full((B, H, D), -777.0, dtype=torch.float16, device=DEV)
        ws = torch.zeros(B * H * splits * (D + 4), dtype=torch.float32, device=DEV)
        cache = (kc.stride(0), kc.stride(1), kc.stride(2), vc.stride(0), vc.stride(1), vc.stride(2))
        m_sb = mask.stride(0) if masked else 0
        sst = _longs(*scales.stride()[:3]) if scales is not None else None
        if form == "two-launch":
            st = _longs(q.stride(0), q.stride(1), *cache, m_sb, out.stride(0), out.stride(1))
            tail = (B, H, HKV, S, D, splits, D ** -0.5, st)
            if fmt == "i8":
                entry = "eetq_decode_attention_i8kv_f16"
                rc = L.eetq_decode_attention_i8kv_f16(_p(q), _p(kc), _p(vc), _p(scales), _p(mask), _p(out), _p(ws), *tail, sst, _p(kv_len),
                                                      0, _p(counter), _stream())
            elif pad:
                entry = "eetq_decode_attention_padded_f16"
                rc = L.eetq_decode_attention_padded_f16(_p(q), _p(kc), _p(vc), _p(mask), _p(out), _p(ws), *tail, _p(kv_len), 0, _p(kv_start),
                                                        _p(counter), _stream())
            else:
                entry = "eetq_decode_attention_f16"
                rc = L.eetq_decode_attention_f16(_p(q), _p(kc), _p(vc), _p(mask), _p(out), _p(ws), *tail, _p(kv_len), 0, _p(counter),
                                                 _stream())
        else:
            st = _longs(q.stride(0), knew.stride(0), vnew.stride(0), *cache, m_sb, out.stride(0), out.stride(1))
            head = (_p(positions), _p(slots), 1, _p(q), _p(knew), _p(vnew), _p(cos_sin), S, _p(kc), _p(vc))
            tail = (_p(mask), _p(out), _p(ws), _p(tickets), B, H, HKV, S, D, splits, D ** -0.5, st)
            if fmt == "i8":
                entry = "eetq_rope_decode_attention_i8kv_f16"
                rc = L.eetq_rope_decode_attention_i8kv_f16(*head, _p(scales), *tail, sst, _p(kv_len), 1, _p(counter), _stream())
            elif pad:
                entry = "eetq_rope_decode_attention_padded_f16"
                rc = L.eetq_rope_decode_attention_padded_f16(*head, *tail, _p(kv_len), 1, _p(kv_start), _p(counter), _stream())
            else:
                entry = "eetq_rope_decode_attention_bounded_f16"
                rc = L.eetq_rope_decode_attention_bounded_f16(*head, *tail, _p(kv_len), 1, _p(counter), _stream())
        torch.cuda.synchronize()
        produced = [out, counter] if form == "two-launch" else [out, kc, vc, tickets, counter] + ([scales] if fmt == "i8" else [])
        digest = _sha(*produced) if rc == 0 else "status=%d" % rc
        tag = ("mask" if masked else "plain") + ("/dropped-step" if drop else "")
        print(entry, D, tag, "LONG" if S > 96 else "short", "S=%d/splits=%d" % (S, splits), digest, flush=True)

    for pad in (False, True):
        for fmt in ("f16",) if pad else ("f16", "i8"):
            for form in ("two-launch", "one-launch"):
                for D in (64, 128):
                    for masked in (False, True):
                        case(fmt, form, D, masked, 96, 2, pad=pad)
                        case(fmt, form, D, masked, 576 if D == 64 else 320, 1, pad=pad)
    for fmt in ("f16", "i8"):
        case(fmt, "one-launch", 128, False, 96, 2, drop=True)
        assert L.eetq_decode_dropped_steps(ctypes.byref(dropped), 1) == 0
        print("eetq_decode_dropped_steps", fmt, dropped.value, flush=True)


if __name__ == "__main__":
    main()
