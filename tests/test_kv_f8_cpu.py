"""What the three C entries of the fp8 KV cache refuse before any launch (include/eetq_amd.h, "The fp8 KV cache"), on a host
without a GPU: EETQ_ERR_INVALID (-1) with the reason, EETQ_ERR_UNSUPPORTED (-3) for a head size other than 64 / 128."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def _args(kind, p, **over):
    """a valid argument list of entry `kind` (B = 1, H = Hkv = 1, S = 8, D = 64), with `over` replacing arguments by name"""
    a = dict(positions=p, slots=None, slot_stride=0, q=p, k=p, v=p, table=p, table_rows=16, kc=p, vc=p, scales=p, mask=None, out=p,
             ws=p, tickets=p, B=1, H=1, Hkv=1, S=8, D=64, splits=1, scaling=0.125, kv_len=None, bias=0, advance=None,
             tokens=2, first_row_dev=None, first_row=0, rot=64)
    a.update(over)
    order = {"decode": "q kc vc scales mask out ws B H Hkv S D splits scaling st kv_len bias advance",
             "rope": "positions slots slot_stride q k v table table_rows kc vc scales mask out ws tickets B H Hkv S D splits scaling "
                     "st kv_len bias advance",
             "write": "positions q k v table table_rows kc vc scales B tokens first_row_dev first_row H Hkv D rot st S"}[kind]
    return [a[n] for n in order.split()] + [None]


@pytest.mark.parametrize("kind", ["decode", "rope", "write"])
def test_fp8_entry_refusals_without_gpu(lib, kind):
    fn = {"decode": lib.eetq_decode_attention_f8kv_f16, "rope": lib.eetq_rope_decode_attention_f8kv_f16,
          "write": lib.eetq_rotary_neox_kvcache_prefill_f8_f16}[kind]
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p, off4, off8 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 8)
    n_st = {"decode": 11, "rope": 12, "write": 6}[kind]
    first_cache = {"decode": 2, "rope": 3, "write": 3}[kind]        # index of the first cache stride
    st = (ctypes.c_long * n_st)(*([64] * n_st))

    def refused(why, **over):
        assert fn(*_args(kind, p, **dict(dict(st=st), **over))) == -1, over
        assert why in lib.eetq_last_error(), (over, lib.eetq_last_error())

    for name in ("q", "kc", "vc", "scales", "st"):
        refused(b"null pointer", **{name: None})
    refused(b"8-byte aligned", kc=off4)
    refused(b"8-byte aligned", vc=off4)
    refused(b"4-byte aligned", scales=ctypes.c_void_p(base + 2))
    refused(b"16-byte aligned", q=off8)
    for i in range(first_cache, first_cache + (3 if kind == "write" else 6)):
        bad = (ctypes.c_long * n_st)(*([64] * n_st))
        bad[i] = 68
        refused(b"multiples of 8 bytes", st=bad)
    bad = (ctypes.c_long * n_st)(*([64] * n_st))
    bad[0] = 60
    refused(b"multiples of 8 elements", st=bad)
    wide = (ctypes.c_long * n_st)(*([64] * n_st))
    wide[first_cache + 2] = 1 << 20                                   # (8 + 4096) rows of 1 MiB: past 2 GiB
    refused(b"less than 2 GiB", st=wide)
    if kind == "rope":
        refused(b"slot_stride", slot_stride=2)
    if kind != "decode":
        refused(b"at least one row", table_rows=0)
    if kind == "write":
        refused(b"rot_dim == head_size", rot=32)
        refused(b"inside the cache", first_row=7)
    assert fn(*_args(kind, p, st=st, D=96, rot=96)) == -3 and b"64 and 128" in lib.eetq_last_error()
