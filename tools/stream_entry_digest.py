"""One call of ops.w8_a16_gemm per point of a fixed, seeded shape list on the dense small-batch launchers (streamk.hip, gemv.hip), one
line per call:

    bits path M N K variant sha256(output bytes)[:16]

Two builds that print the same lines compute the same bits on every branch the launchers take by default on a 256-CU MI355X: the
register, block-copy and ring forms of the stream kernel with one and two tile rows per workgroup and 8 and 16 waves, its shallow-K
forms, the 32-row ring and the three- and four-tile register forms of the explicit path, the GEMV's straight-line, generic and
column-unit forms with their plain, epilogue and prologue instantiations.  A wrong wave count changes the summation order and so the
digest; a wrong form at an equal wave count does not -- `rocprofv3 --kernel-trace --stats -- python tools/stream_entry_digest.py`
gives the kernel each call launches.  Needs an MI355X.

    python tools/stream_entry_digest.py > digest.txt
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
M_STREAM = {8: (1, 2, 4, 5, 8, 9, 12, 16, 17, 32, 33, 48, 64), 4: (1, 2, 4, 5, 8, 9, 12, 16)}
M_GEMV = (1, 2, 3, 4)
# (N, K): the smallest pairs that reach each branch on 256 CUs -- 1 / 1+ / 1.25 / 2 / 2.7 / 3.5 / 5.4 tile rows per CU at K = 4096 and
# 8192, the shallow-K forms, a quarter of the CUs, the GEMV's column units (5120 x 13824: 8 + 8 + 4 columns per CU)
SHAPES = [(N, K) for K in (4096, 8192) for N in (4096, 4112, 5120, 8192, 11008, 14336, 22016)] + \
         [(4096, 64), (4096, 256), (4096, 1024), (4096, 2048), (1024, 8192), (5120, 13824)]
MAX_N, MAX_K, MAX_M = 22016, 13824, 64
# (N, K), 16384 <= K <= 32768, for the GEMV launchers alone (M * K <= 65536: what they stage in LDS): the column units with eight
# activation loads per thread (64 x 28672, 64 x 32768; 5120 x 28672: 8 + 8 + 4), the 16-wave generic form with four (64 x 28736, K / 64
# odd) and the 8-wave one with four and eight (8208 x 16384 / 28672 / 32768: 513 tile rows), M = 4 at its deepest K (64 x 16384)
DEEP_SHAPES = [(64, 16384), (8208, 16384), (64, 28672), (5120, 28672), (8208, 28672), (64, 28736), (64, 32768), (8208, 32768)]
DEEP_N, DEEP_K = 8208, 32768


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def main():
    assert torch.cuda.is_available(), "tools/stream_entry_digest.py needs a GPU"
    from eetq_amd import ops
    g = torch.Generator().manual_seed(12)
    # any bytes are valid weights (int8 [K, N], or int4 pairs [K, N / 2]): every shape takes a prefix of one pool
    wpool = torch.randint(-128, 128, (8192 * MAX_N,), dtype=torch.int8, generator=g).to(DEV)
    spool = (torch.rand(MAX_N, generator=g) * 1e-3 + 1e-4).half().to(DEV)
    spool = {8: spool, 4: spool * 16}
    xpool = torch.randn(MAX_M * MAX_K, generator=g).half().to(DEV)
    bpool = torch.randn(MAX_N, generator=g).half().to(DEV)
    rpool = torch.randn(MAX_M * MAX_N, generator=g).half().to(DEV)
    gamma = (torch.rand(MAX_K, generator=g) + 0.5).half().to(DEV)
    # (drawn after everything above, so the lines of SHAPES do not depend on the deep pools)
    wdeep = torch.randint(-128, 128, (DEEP_K * DEEP_N,), dtype=torch.int8, generator=g).to(DEV)
    gamma_deep = (torch.rand(DEEP_K, generator=g) + 0.5).half().to(DEV)

    def emit(bits, path, M, N, K, variant, **kw):
        nb = N // 2 if bits == 4 else N
        w = (wdeep if K > MAX_K else wpool)[:K * nb].view(K, nb)
        x = xpool[:M * K * (2 if kw.get("gated") else 1)].view(M, -1)
        y = ops.w8_a16_gemm(x, w, spool[bits][:N], path, **kw)
        assert bool(torch.isfinite(y.float()).all()), (bits, path, M, N, K, variant)
        print(bits, path, M, N, K, variant, _sha(y), flush=True)

    with torch.no_grad():
        for bits in (8, 4):
            for path, ms in (("stream", M_STREAM[bits]), ("gemv", M_GEMV), ("auto", M_GEMV)):
                for N, K in SHAPES:
                    if bits == 4 and K % 128:
                        continue
                    for M in ms:
                        emit(bits, path, M, N, K, "plain")
                        emit(bits, path, M, N, K, "bias+residual", bias=bpool[:N], residual=rpool[:M * N].view(M, N))
                        if bits == 8 and path == "auto":   # the gated epilogue: GEMV at one row, the stream kernel above
                            emit(bits, path, M, N, K, "silu_glu8", activation="silu_glu8")
                        if bits == 8 and path == "auto" and M == 1:   # the GEMV's prologue instantiations
                            emit(bits, path, M, N, K, "norm", norm=(gamma[:K], 1e-5))
                            emit(bits, path, M, N, K, "gated", gated=True)
            for path in ("gemv", "auto"):
                for N, K in DEEP_SHAPES:
                    if bits == 4 and K % 128:
                        continue
                    for M in M_GEMV:
                        if M * K > 65536:
                            continue
                        emit(bits, path, M, N, K, "plain")
                        emit(bits, path, M, N, K, "bias+residual", bias=bpool[:N], residual=rpool[:M * N].view(M, N))
                        if bits == 8 and path == "auto" and M == 1:
                            emit(bits, path, M, N, K, "silu_glu8", activation="silu_glu8")
                            emit(bits, path, M, N, K, "norm", norm=(gamma_deep[:K], 1e-5))
                            emit(bits, path, M, N, K, "gated", gated=True)


if __name__ == "__main__":
    main()
