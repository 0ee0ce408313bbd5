"""The small-batch plan (eetq_diag_stream_plan: streamk.hip::resolve with empty overrides) over a grid of shapes, one line per
(bits, cus):

    bits cus points sha256("M N K form tile_rows waves\\n" ...)

Host arithmetic only, no GPU.  Two builds that print the same lines pick the same plan at every point of the grid:
  M   1 .. 16
  N   16 r, r on and two either side of 1, 1.5, 2, 3 and 4 tile rows per CU (both parities of r)
  K   every multiple of the tile depth (64 / 128) up to 2048, then a ladder to 32768 around the rules' K thresholds

    python tools/stream_plan_digest.py > digest.txt
"""
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LADDER = (2560, 3072, 3584, 4096, 4096 + 64, 4096 + 128, 5120 - 128, 5120, 6144, 6144 + 64, 6144 + 128, 7168, 8192 - 128, 8192,
          8192 + 64, 8192 + 128, 9216, 10240, 11008, 12288, 13824, 16384, 24576, 28672, 32768 - 128, 32768)


def grid(bits, cus):
    tile_k = 128 if bits == 4 else 64
    ks = list(range(tile_k, 2048 + 1, tile_k)) + [k for k in LADDER if k % tile_k == 0]
    rs = sorted({int(q * cus) + d for q in (1, 1.5, 2, 3, 4) for d in (-2, -1, 0, 1, 2)})
    for M in range(1, 17):
        for r in rs:
            for K in ks:
                yield M, 16 * r, K


def main():
    from eetq_amd import _lib
    lib = _lib.lib()
    f, t, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for bits in (4, 8):
        for cus in (64, 128, 256, 304):
            h, n = hashlib.sha256(), 0
            for M, N, K in grid(bits, cus):
                rc = lib.eetq_diag_stream_plan(bits, M, N, K, cus, ctypes.byref(f), ctypes.byref(t), ctypes.byref(w))
                assert rc == 0, (bits, cus, M, N, K)
                h.update(b"%d %d %d %d %d %d\n" % (M, N, K, f.value, t.value, w.value))
                n += 1
            print(bits, cus, n, h.hexdigest(), flush=True)


if __name__ == "__main__":
    main()
