"""eetq_diag_tile_plan with cus <= 0 asks the device: an MI355X has 256 CUs, so both calls agree (tests/test_tile_plan_cpu.py pins
the plans themselves without a device)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu


def test_device_cu_count_reaches_the_planner():
    from eetq_amd import _lib
    lib = _lib.lib()
    assert lib.eetq_device_supported() == 1, "kernels are built for gfx950 only"
    for bits in (8, 4):
        for M, N, K in ((200, 384, 1024), (1024, 2176, 384), (1024, 5120, 384), (1024, 5120, 5120)):
            got = []
            for cus in (0, 256):
                rec, count = (ctypes.c_int * 24)(*([-9] * 24)), ctypes.c_int(-9)
                assert lib.eetq_diag_tile_plan(bits, M, N, K, 0, 0, cus, rec, 4, ctypes.byref(count)) == 0, (bits, M, N, K, cus)
                got.append((count.value, list(rec)))
            assert got[0] == got[1] and 1 <= got[0][0] <= 2, (bits, M, N, K, got)
