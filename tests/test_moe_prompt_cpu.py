"""The prompt path of the routed experts without a GPU: eetq_w8a16_moe_gemm_tiled is declared, exported and
prototyped within ABI revision 7 and refuses every bad argument eetq_w8a16_moe_gemm refuses before any launch; the grouped
instantiations of the tile kernel feed LDS-DMA stages into 32x32x16 MFMAs without scratch or spills; the shape-only slot bound
floor(S / 128) + min(E, S) holds for random and adversarial expert counts and the slot -> (expert, row tile) map covers every
sorted row exactly once."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "eetq_w8a16_moe_gemm_tiled"
ERR_INVALID = -1
LLVM_BIN = "/opt/rocm/lib/llvm/bin"
BM = 128


@pytest.fixture(scope="module")
def lib():
    from eetq_amd import _lib
    return _lib.lib()


def test_entry_declared_exported_and_prototyped(lib):
    from eetq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "eetq_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NEW, hdr)
    assert NEW in _lib.EXPORTED_SYMBOLS
    assert getattr(lib, NEW).argtypes == lib.eetq_w8a16_moe_gemm.argtypes   # the decode entry's signature
    assert "#define EETQ_AMD_ABI_VERSION 7" in hdr
    assert lib.eetq_abi_version() == 7


@pytest.mark.parametrize("entry", ["eetq_w8a16_moe_gemm", NEW])
def test_rejects_bad_arguments_before_any_launch(lib, entry):
    fn = getattr(lib, entry)
    p, n = ctypes.c_void_p(16), None
    # x, w, scales, offsets, sorted_slot, active, y, T, k, E, N, K, gather, glu8, stream
    ok = [p, p, p, p, p, p, p, 64, 2, 8, 256, 512, 1, 0, n]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return fn(*a)

    for i in range(7):                                                        # every pointer (sorted_slot: needed when gathering)
        assert call(**{"a%d" % i: n}) == ERR_INVALID, i
        assert entry.encode() + b": null pointer" in lib.eetq_last_error()
    assert call(a9=0) == ERR_INVALID and call(a9=1025) == ERR_INVALID         # E
    assert call(a8=0) == ERR_INVALID and call(a8=9) == ERR_INVALID            # k
    assert call(a7=0) == ERR_INVALID and call(a7=1 << 30) == ERR_INVALID      # T
    assert call(a11=500) == ERR_INVALID and b"K % 64" in lib.eetq_last_error()
    assert call(a10=200) == ERR_INVALID and b"N % 16" in lib.eetq_last_error()
    assert call(a12=2) == ERR_INVALID and call(a13=-1) == ERR_INVALID         # gather, glu8
    for i in (0, 1, 6):                                                       # x, weight, y alignment
        assert call(**{"a%d" % i: ctypes.c_void_p(24)}) == ERR_INVALID, i
        assert b"aligned" in lib.eetq_last_error()


def test_ctypes_binding_still_refuses_the_layer():
    from eetq_amd import ops_ctypes
    with pytest.raises(RuntimeError, match="compiled EETQ module"):
        ops_ctypes.w8_a16_moe(None, None, None, None, None, None, None)


def _device_object(tmp_path):
    objdump = os.path.join(LLVM_BIN, "llvm-objdump")
    if not os.path.exists(objdump):
        objdump = shutil.which("llvm-objdump")
    assert objdump, "llvm-objdump not found"
    local = os.path.join(str(tmp_path), "moe_gemm_tiled.o")
    shutil.copy(os.path.join(ROOT, "eetq_amd", "csrc", "moe_gemm_tiled.o"), local)
    subprocess.run([objdump, "--offloading", local], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    dev = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(str(tmp_path))
    return objdump, os.path.join(str(tmp_path), dev[0])


def test_grouped_tile_kernels_machine_code(lib, tmp_path):
    objdump, dev = _device_object(tmp_path)
    text = subprocess.run([objdump, "-d", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    # moe_gemm_tile_kernel<J, GLU>: J = 1, 2 x plain, GLU (Itanium mangling ILi<J>ELb<GLU>E)
    syms = re.findall(r"<(_Z\w*moe_gemm_tile_kernelILi[12]ELb[01]E\w*)>:", text)
    assert len(syms) == 4 and len(set(syms)) == 4, syms
    readelf = os.path.join(LLVM_BIN, "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found"
    notes = subprocess.run([readelf, "--notes", dev], check=True, stdout=subprocess.PIPE, text=True).stdout
    for sym in syms:
        body = text.split("<%s>:" % sym, 1)[1].split("\n\n", 1)[0]
        assert re.search(r"\bv_mfma_f32_32x32x16_f16\b", body), sym
        assert re.search(r"\bbuffer_load_dwordx4\b.*\blds\b", body), sym    # the LDS-DMA stage loads
        assert not re.search(r"\bscratch_", body), sym
        meta = [k for k in re.split(r"\n\s*- \.", notes) if sym in k]
        assert meta, "no code-object metadata for %s" % sym
        for k in meta:
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", k), k
            assert re.search(r"\.vgpr_spill_count:\s+0\b", k), k
            assert re.search(r"\.sgpr_spill_count:\s+0\b", k), k


# ---- the slot bound and the slot map, restated in Python -------------------------------------------------------------------------
def _slot_map(counts, S):
    """what a workgroup of gemm_tile_body<GROUPED> computes: slot r -> (expert, first row, rows) or None for a surplus slot"""
    E = len(counts)
    A = min(E, S)
    active = [e for e in range(E) if counts[e] > 0]
    assert len(active) <= A
    active += [-1] * (A - len(active))
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + c)
    R = S // BM + A
    per = (A + 63) >> 6
    mine = []
    for lane in range(64):
        m = 0
        for i in range(per):
            a = lane * per + i
            e = active[a] if a < A else -1
            if e >= 0:
                m += (offsets[e + 1] - offsets[e] + BM - 1) // BM
        mine.append(m)
    out = []
    for slot in range(R):
        inc, hit = 0, None
        for lane in range(64):
            first = inc
            inc += mine[lane]
            if first <= slot < inc and hit is None:
                hit = (lane, first)
        if hit is None:
            out.append(None)
            continue
        lane, t = hit
        found = None
        for i in range(per):
            a = lane * per + i
            e = active[a] if a < A else -1
            n = (offsets[e + 1] - offsets[e] + BM - 1) // BM if e >= 0 else 0
            if slot < t + n:
                found = (e, t)
                break
            t += n
        assert found is not None
        e, t0 = found
        m0 = (slot - t0) * BM
        rows = min(BM, counts[e] - m0)
        assert rows >= 1
        out.append((e, offsets[e] + m0, rows))
    return R, out


def _count_vectors():
    rnd = random.Random(7)
    cases = []
    for E, S in ((8, 34), (8, 128), (8, 8192), (128, 512), (128, 136), (128, 32768), (1024, 100), (1024, 4096), (3, 2), (1, 300)):
        A = min(E, S)
        cases.append((E, S, [S] + [0] * (E - 1)))                                   # every slot on one expert
        cases.append((E, S, [0] * (E - 1) + [S]))
        one_each = [1] * A + [0] * (E - A)                                          # one row on each of min(E, S) experts, the rest ...
        one_each[0] += S - A                                                        # ... on the first
        cases.append((E, S, one_each))
        cases.append((E, S, [1] * A + [0] * (E - A)))                               # sentinels took the rest: sum < S
        cases.append((E, S, [0] * E))                                               # nothing routed at all
        for _ in range(6):                                                          # random, with sentinels
            used = rnd.randint(0, S)
            c = [0] * E
            for _ in range(used):
                c[rnd.randrange(E)] += 1
            cases.append((E, S, c))
        for base in (127, 128, 129):                                                # counts straddling the tile height
            c, left = [0] * E, S
            for e in range(E):
                take = min(left, base + rnd.choice((-1, 0, 1)))
                c[e] = take
                left -= take
            cases.append((E, S, c))
    return cases


def test_slot_bound_and_slot_map_cover_every_row_once():
    for E, S, counts in _count_vectors():
        assert sum(counts) <= S
        tiles = sum((c + BM - 1) // BM for c in counts)
        R, slots = _slot_map(counts, S)
        assert R == S // BM + min(E, S)
        assert tiles <= R, (E, S, counts)
        live = [s for s in slots if s is not None]
        assert len(live) == tiles
        assert all(s is None for s in slots[tiles:])                               # live slots first, surplus slots after them
        seen = [0] * sum(counts)
        offsets = [0]
        for c in counts:
            offsets.append(offsets[-1] + c)
        for e, p, rows in live:
            assert offsets[e] <= p and p + rows <= offsets[e + 1]                   # never past the expert's count
            for r in range(p, p + rows):
                seen[r] += 1
        assert all(v == 1 for v in seen), (E, S, counts)
