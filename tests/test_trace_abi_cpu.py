"""Host-side contract of itsd_sampler_set_trace: the symbol is exported and bound, and a null handle is refused with
ITSD_ERR_INVALID and a message naming the function before any device call (so this runs without a GPU). The refusals
that need a UNet handle (no x0-form schedule, rows != T_sched, stride < 1, a misaligned pointer, n > stride, a
straddling geometry) are in tests/test_gpu_x0_trace.py."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from itsd import runtime as rt


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def test_symbol_exported_and_bound(L):
    lib = ctypes.CDLL(rt.LIB_PATH)
    assert hasattr(lib, "itsd_sampler_set_trace"), "missing export itsd_sampler_set_trace"
    assert "itsd_sampler_set_trace" in rt.EXPORTS
    assert hasattr(rt.NativeUNet, "set_trace")
    src = open(os.path.join(ROOT, "include", "itsd.h")).read()
    assert re.search(r"^int\s+itsd_sampler_set_trace\s*\(itsd_unet\* u, double\* trace, int rows, int stride\);", src,
                     re.M)


@pytest.mark.parametrize("trace", [0x10000, None])  # attach and detach alike
def test_null_handle(L, trace):
    rc = L.itsd_sampler_set_trace(None, trace, 6, 4)
    msg = L.itsd_last_error().decode()
    assert rc == rt.ITSD_ERR_INVALID
    assert "itsd_sampler_set_trace" in msg and "null handle" in msg


def test_query_null_handle_still_refused(L):
    v = ctypes.c_int64(7)
    assert L.itsd_unet_query(None, b"trace", ctypes.byref(v)) == rt.ITSD_ERR_INVALID
