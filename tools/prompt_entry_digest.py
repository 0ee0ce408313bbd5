"""One call of every form of the prompt-side C entries (eetq_amd/csrc/attn_prefill.hip, attn_decode_rows.hip and the prompt cache
writes of norm_rope.hip) on seeded inputs, one line per call:

    entry D case sha256(everything the call produces)

"Everything" is the output of an attention entry; of a cache write the rotated query and key, both caches whole (the written rows,
and any row that should not have been) and the scale tensor of an int8 cache.  A call the entry refuses prints its status and the
library's error text instead.  Covered:
  * eetq_prefill_attention_f16 / _dev_f16 / _padded_f16 / _i8kv_f16: two batch rows, 4 heads on 2 kv heads, D {64, 128}, a 200-row
    cache whose heads are NOT contiguous, 167 keys from a device length (three key blocks, the last partial) or all 200 from the
    host, Tq {3, 130} (130: two query blocks, the second with two real rows), splits {1, 2}, kv_start [3, 40] in the padded form;
  * eetq_decode_attention_rows_f16: query tiles of 4, 32, 48, 64 and 80 rows (1 .. 4 sub-tiles and a second tile group), splits {1, 3};
  * eetq_rotary_neox_kvcache_prefill_bounded_f16 / _prefill_i8_f16: T {1, 5}, the first row from the host and from the device;
  * one refused call per requirement the launchers share: splits 0 and beyond the maximum, a misaligned workspace, a q stride of 4,
    max_keys 0, a null kv_start.
Two builds of the library that print the same lines compute the same bits through every entry.  Needs an MI355X.

    python tools/prompt_entry_digest.py [--lib OTHER/libeetq_amd.so] > digest.txt
"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
B, HKV, S, FILLED = 2, 2, 200, 167
ENTRIES = ("eetq_prefill_attention_f16", "eetq_prefill_attention_dev_f16", "eetq_prefill_attention_padded_f16",
           "eetq_prefill_attention_i8kv_f16", "eetq_prefill_attention_workspace_floats", "eetq_decode_attention_rows_f16",
           "eetq_decode_attention_rows_workspace_floats", "eetq_rotary_neox_kvcache_prefill_bounded_f16",
           "eetq_rotary_neox_kvcache_prefill_i8_f16", "eetq_last_error")


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
    assert torch.cuda.is_available(), "tools/prompt_entry_digest.py needs a GPU"
    from eetq_amd import _lib
    L = _lib.lib()
    if args.lib:
        other = ctypes.CDLL(os.path.abspath(args.lib))
        for name in ENTRIES:
            getattr(other, name).argtypes = getattr(L, name).argtypes
            getattr(other, name).restype = getattr(L, name).restype
        L = other
    g = torch.Generator().manual_seed(43)

    def half(*shape):
        return (torch.rand(*shape, generator=g) - 0.5).half().to(DEV)

    def caches(fmt, D):
        """[B, Hkv, S, D] views of [B, S, Hkv, D] storage: a head's rows are Hkv * D apart"""
        if fmt == "f16":
            return half(B, S, HKV, D).transpose(1, 2), half(B, S, HKV, D).transpose(1, 2), None
        kc = torch.randint(-127, 128, (B, S, HKV, D), dtype=torch.int8, generator=g).to(DEV).transpose(1, 2)
        vc = torch.randint(-127, 128, (B, S, HKV, D), dtype=torch.int8, generator=g).to(DEV).transpose(1, 2)
        return kc, vc, (torch.rand(B, S, HKV, 2, generator=g) * 4e-3 + 1e-4).half().to(DEV).transpose(1, 2)

    def report(entry, D, tag, rc, *produced):
        torch.cuda.synchronize()
        print(entry, D, tag, _sha(*produced) if rc == 0 else "status=%d %s" % (rc, L.eetq_last_error().decode()), flush=True)

    def prompt(form, D, Tq, splits, dev_len, H=4, refuse=None):
        """form: host / dev / padded / i8kv / rows (Tq = its R); refuse: the one argument made invalid"""
        fmt = "i8" if form == "i8kv" else "f16"
        q = half(B, Tq, 3 * H, D)[:, :, :H]   # the query third of a fused projection: tokens 3 H D apart
        kc, vc, scales = caches(fmt, D)
        out = torch.full((B, Tq, H, D), -777.0, dtype=torch.float16, device=DEV)
        kv_len = torch.tensor([FILLED], dtype=torch.int64, device=DEV) if dev_len else None
        kv_start = torch.tensor([3, 40], dtype=torch.int64, device=DEV)
        max_keys = 0 if refuse == "max_keys" else S
        if refuse in ("splits-low", "splits-high"):
            splits = 0 if refuse == "splits-low" else (65 if form == "rows" else 17)
        floats = L.eetq_decode_attention_rows_workspace_floats if form == "rows" else L.eetq_prefill_attention_workspace_floats
        need = int(floats(B, H, Tq, D, max(splits, 2 if refuse == "workspace" else 1)))
        ws = torch.zeros(need + 4, dtype=torch.float32, device=DEV)[1 if refuse == "workspace" else 0:] if need else None
        st = [*q.stride()[:3], *kc.stride()[:3], *vc.stride()[:3], *out.stride()[:3]]
        if refuse == "q-stride":
            st[2] = 4
        st, sc = _longs(*st), D ** -0.5
        dims = (B, H, HKV, Tq, max_keys, D)
        dev_tail = (_p(kv_len), 0, splits, sc, st)
        if form == "host":
            keys = min(FILLED, max_keys) if dev_len else max_keys   # the host form's length is an argument
            entry = "eetq_prefill_attention_f16"
            rc = L.eetq_prefill_attention_f16(_p(q), _p(kc), _p(vc), _p(out), B, H, HKV, Tq, keys, D, keys - Tq, sc, st, _stream())
        elif form == "dev":
            entry = "eetq_prefill_attention_dev_f16"
            rc = L.eetq_prefill_attention_dev_f16(_p(q), _p(kc), _p(vc), _p(out), _p(ws), *dims, *dev_tail, _stream())
        elif form == "padded":
            entry = "eetq_prefill_attention_padded_f16"
            rc = L.eetq_prefill_attention_padded_f16(_p(q), _p(kc), _p(vc), _p(out), _p(ws), *dims, _p(kv_len), 0,
                                                     _p(None if refuse == "kv_start" else kv_start), splits, sc, st, _stream())
        elif form == "i8kv":
            entry = "eetq_prefill_attention_i8kv_f16"
            rc = L.eetq_prefill_attention_i8kv_f16(_p(q), _p(kc), _p(vc), _p(scales), _p(out), _p(ws), *dims, *dev_tail,
                                                   _longs(*scales.stride()[:3]), _stream())
        else:
            entry = "eetq_decode_attention_rows_f16"
            rc = L.eetq_decode_attention_rows_f16(_p(q), _p(kc), _p(vc), _p(out), _p(ws), *dims, *dev_tail, _stream())
        tag = "refused:" + refuse if refuse else "H=%d/Tq=%d/splits=%d/%s" % (H, Tq, splits, "kv_len=%d" % FILLED if dev_len else "host-length")
        report(entry, D, tag, rc, out)

    def rotary(fmt, D, T, from_device, H=4):
        q, k, v = half(B, T, H, D), half(B, T, HKV, D), half(B, T, HKV, D)
        kc, vc, scales = caches(fmt, D)
        assert vc.stride() == kc.stride()   # the fp16 entry takes one set of cache strides
        first = 7
        positions = (torch.arange(T)[None, :] + torch.tensor([[first], [first + 20]])).to(torch.int64).to(DEV)
        theta = torch.rand(256, D // 2, generator=g) * 6.0
        table = torch.cat([theta.cos(), theta.sin()], dim=1).half().to(DEV)
        first_dev = torch.tensor([first + 4], dtype=torch.int64, device=DEV) if from_device else None
        st = _longs(q.stride(1), k.stride(1), v.stride(1), *kc.stride()[:3])
        head = (_p(positions), _p(q), _p(k), _p(v), _p(table), table.shape[0], _p(kc), _p(vc))
        tail = (B, T, _p(first_dev), first, H, HKV, D, D, st)
        if fmt == "f16":
            entry = "eetq_rotary_neox_kvcache_prefill_bounded_f16"
            rc = L.eetq_rotary_neox_kvcache_prefill_bounded_f16(*head, *tail, S, _stream())
        else:
            entry = "eetq_rotary_neox_kvcache_prefill_i8_f16"
            rc = L.eetq_rotary_neox_kvcache_prefill_i8_f16(*head, _p(scales), *tail, _longs(*scales.stride()[:3]), S, _stream())
        tag = "T=%d/first_row=%s" % (T, "device" if from_device else "host")
        report(entry, D, tag, rc, q, k, kc, vc, *([scales] if fmt == "i8" else []))

    for form in ("host", "dev", "padded", "i8kv"):
        for D in (64, 128):
            for Tq in (3, 130):
                for splits in (1,) if form == "host" else (1, 2):
                    for dev_len in (True, False):
                        prompt(form, D, Tq, splits, dev_len)
    for groups, R in ((2, 2), (2, 16), (4, 12), (4, 16), (8, 10)):   # tiles of 4, 32, 48, 64, 80 rows
        for D in (64, 128):
            for splits in (1, 3):
                for dev_len in (True, False):
                    prompt("rows", D, R, splits, dev_len, H=groups * HKV)
    for fmt in ("f16", "i8"):
        for D in (64, 128):
            for T in (1, 5):
                for from_device in (False, True):
                    rotary(fmt, D, T, from_device)
    for form in ("host", "dev", "padded", "i8kv", "rows"):
        for refuse in ("splits-low", "splits-high", "workspace", "q-stride", "max_keys", "kv_start"):
            if refuse == "kv_start" and form != "padded":
                continue
            if form == "host" and refuse not in ("q-stride", "max_keys"):
                continue
            prompt(form, 64, 3, 2, True, refuse=refuse)


if __name__ == "__main__":
    main()
