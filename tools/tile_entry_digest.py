"""One call of every C entry point that launches the LDS-tiled MFMA kernel (gemm_tile_body) through the shared launch plan
(eetq_amd/csrc/gemm_tile_plan.hpp), on seeded inputs, one line per call:

    entry bits M N K variant sha256(output bytes)

Every call is made twice -- a warm-up call, then the call whose output is hashed; a call the entry refuses prints its status
instead of a hash.  Two builds of the library that print the same lines compute the same bits on every branch of the plan: the
single narrow or wide launch, the seam between whole rounds of wide tiles and the ragged round (with the bias / residual offsets
crossing it), that round in two K slices, the stream kernel below K = 320, the forced K slices and their fall-back, the int4 tile at
its rule and at both forced shapes, and both grouped forms at both tile shapes with and without the gather and the GLU write-out.
Grouped lines carry M = T k.  Needs an MI355X.

    python tools/tile_entry_digest.py > digest.txt
"""
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
POISON = -777.0


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _emit(entry, bits, M, N, K, variant, out, call):
    for _ in range(2):
        out.fill_(POISON)
        rc = call()
        torch.cuda.synchronize()
    digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() if rc == 0 else "status=%d" % rc
    print(entry, bits, M, N, K, variant, digest, flush=True)


def _dense_inputs(g, bits, M, N, K):
    """any bytes are a valid weight in either tile layout: int8 [K][N], int4 pairs [K][N / 2]"""
    x = (torch.rand(M, K, generator=g) - 0.5).half().to(DEV)
    w = torch.randint(-128, 128, (K, N * bits // 8), dtype=torch.int8, generator=g).to(DEV)
    s = (torch.rand(N, generator=g) * (2e-2 if bits == 4 else 1e-3) + 1e-4).half().to(DEV)
    bias = (torch.rand(N, generator=g) - 0.5).half().to(DEV)
    res = (torch.rand(M, N, generator=g) - 0.5).half().to(DEV)
    return x, w, s, bias, res


def main():
    assert torch.cuda.is_available(), "tools/tile_entry_digest.py needs a GPU"
    from eetq_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(23)

    def w8(path, M, N, K, variant, bias=False, res=False, act=_lib.ACT_IDENTITY):
        x, w, s, b, r = _dense_inputs(g, 8, M, N, K)
        y = torch.empty(M, N, dtype=torch.float16, device=DEV)
        name = "eetq_w8a16_gemm_ex(%s)" % {_lib.PATH_MFMA: "MFMA", _lib.PATH_TILESPLIT: "TILESPLIT"}[path]
        _emit(name, 8, M, N, K, variant, y, lambda: L.eetq_w8a16_gemm_act(_p(x), _p(w), _p(s), _p(b if bias else None), _p(r if res else None),
                                                                          _p(y), M, N, K, path, act, _stream()))

    w8(_lib.PATH_MFMA, 200, 384, 1024, "plain")
    w8(_lib.PATH_MFMA, 200, 384, 1024, "bias+residual", bias=True, res=True)
    w8(_lib.PATH_MFMA, 200, 384, 1024, "gelu", bias=True, act=_lib.ACT_GELU)
    for M, N, K in ((200, 384, 1024), (1024, 22016, 4096)):   # the second: a shape AUTO runs on the unsplit tile, so the write-out runs
        x, w, s, b, _ = _dense_inputs(g, 8, M, N, K)
        y = torch.empty(M, N // 2, dtype=torch.float16, device=DEV)
        _emit("eetq_w8a16_gemm_glu8", 8, M, N, K, "glu8", y, lambda: L.eetq_w8a16_gemm_glu8(_p(x), _p(w), _p(s), _p(b), _p(y), M, N, K, _stream()))
    w8(_lib.PATH_MFMA, 1024, 2176, 384, "plain")
    w8(_lib.PATH_MFMA, 1024, 5120, 384, "bias+residual", bias=True, res=True)
    w8(_lib.PATH_MFMA, 1024, 5120, 384, "relu", bias=True, act=_lib.ACT_RELU)
    w8(_lib.PATH_MFMA, 1024, 5120, 5120, "plain")
    w8(_lib.PATH_MFMA, 1024, 5120, 5120, "bias+residual", bias=True, res=True)
    w8(_lib.PATH_MFMA, 130, 256, 272, "residual", res=True)    # K % 64 != 0: the entry refuses it
    w8(_lib.PATH_MFMA, 130, 256, 256, "residual", res=True)    # the stream kernel over 64-row chunks
    w8(_lib.PATH_TILESPLIT, 128, 4096, 11008, "plain")
    w8(_lib.PATH_TILESPLIT, 512, 4096, 11008, "bias+residual", bias=True, res=True)
    w8(_lib.PATH_TILESPLIT, 200, 384, 1024, "plain")

    for M, N, K, fused in ((200, 384, 1024, False), (1024, 2176, 384, False), (1024, 5120, 384, True)):
        x, w, s, b, r = _dense_inputs(g, 4, M, N, K)
        y = torch.empty(M, N, dtype=torch.float16, device=DEV)
        for tile_j in (0, 1, 2):
            _emit("eetq_w4a16_gemm_tiled", 4, M, N, K, ("bias+residual" if fused else "plain") + "/tile_j=%d" % tile_j, y,
                  lambda: L.eetq_w4a16_gemm_tiled(_p(x), _p(w), _p(s), _p(b if fused else None), _p(r if fused else None), _p(y), M, N, K,
                                                  tile_j, _stream()))

    T, k, E = 330, 2, 4
    S = T * k
    idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(DEV)
    tables = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (E, E + 1, S, S, min(E, S))]
    assert L.eetq_moe_route(_p(idx), T, k, E, *[_p(t) for t in tables], _stream()) == 0
    _, offsets, sorted_slot, _, active = tables
    for N, K in ((384, 384), (768, 384)):
        for bits in (8, 4):
            w = torch.randint(-128, 128, (E, K, N * bits // 8), dtype=torch.int8, generator=g).to(DEV)
            s = (torch.rand(E, N, generator=g) * (2e-2 if bits == 4 else 1e-3) + 1e-4).half().to(DEV)
            for gather in (1, 0):
                x = (torch.rand(T if gather else S, K, generator=g) - 0.5).half().to(DEV)
                for glu8 in (0, 1):
                    y = torch.empty(S, N // 2 if glu8 else N, dtype=torch.float16, device=DEV)
                    args = (_p(x), _p(w), _p(s), _p(offsets), _p(sorted_slot), _p(active), _p(y), T, k, E, N, K, gather, glu8)
                    tag = "gather=%d/glu8=%d" % (gather, glu8)
                    if bits == 8:
                        _emit("eetq_w8a16_moe_gemm_tiled", 8, S, N, K, tag, y, lambda: L.eetq_w8a16_moe_gemm_tiled(*args, _stream()))
                        continue
                    for tile_j in (0, 1, 2):
                        _emit("eetq_w4a16_moe_gemm_tiled", 4, S, N, K, tag + "/tile_j=%d" % tile_j, y,
                              lambda: L.eetq_w4a16_moe_gemm_tiled(*args, tile_j, _stream()))


if __name__ == "__main__":
    main()
