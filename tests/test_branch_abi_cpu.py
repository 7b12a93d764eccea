"""Host-side contract of the two entry points of the branching path search, itsd_sampler_predict_x0 and
itsd_branch: both are exported, and every invalid-argument case that needs no UNet handle is refused with
ITSD_ERR_INVALID and a message before any device call (so this runs without a GPU). Pointers are plain integers:
a refused call never dereferences a device pointer."""
import ctypes
import os

import pytest

from itsd import runtime as rt


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def _parents(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _refused(L, rc):
    assert rc == rt.ITSD_ERR_INVALID
    assert L.itsd_last_error().decode()  # a message, not an empty string


def _branch(L, dst=0x10000, src=0x20000, parents=_parents(0, 0), n_src=1, n_dst=2, per=4, a=1.0, b=0.5):
    return L.itsd_branch(dst, src, parents, n_src, n_dst, per, a, b, 1, 2, 0, None)


def test_symbols_exported_and_bound(L):
    lib = ctypes.CDLL(rt.LIB_PATH)
    for name in ("itsd_sampler_predict_x0", "itsd_branch"):
        assert hasattr(lib, name), f"missing export {name}"
        assert name in rt.EXPORTS


def test_branch_null_pointers(L):
    _refused(L, _branch(L, dst=None))
    _refused(L, _branch(L, src=None))
    _refused(L, _branch(L, parents=None))


def test_branch_counts_and_sizes(L):
    _refused(L, _branch(L, per=0))
    _refused(L, _branch(L, per=-4))
    _refused(L, _branch(L, n_dst=-1))
    _refused(L, _branch(L, n_src=-1))
    _refused(L, _branch(L, n_src=0))


def test_branch_parent_out_of_range(L):
    _refused(L, _branch(L, n_src=3, parents=_parents(0, 3)))   # == n_src
    _refused(L, _branch(L, n_src=3, parents=_parents(-1, 0)))
    _refused(L, _branch(L, n_src=3, n_dst=3, parents=_parents(2, 1, 7)))


def test_branch_overlapping_ranges(L):
    per, n_src, n_dst = 4, 3, 2  # src: 48 bytes, dst: 32 bytes
    src = 0x40000
    for dst in (src, src + 16, src + 3 * per * 4 - 4, src - 2 * per * 4 + 4, src - 16):
        _refused(L, _branch(L, dst=dst, src=src, n_src=n_src, n_dst=n_dst, per=per, parents=_parents(0, 2)))


def test_branch_zero_rows_is_a_noop(L):
    assert _branch(L, n_dst=0) == rt.ITSD_OK
    # (nothing is launched: the dst / src integers above are not device memory)
    assert _branch(L, n_dst=0, n_src=5, parents=_parents(0)) == rt.ITSD_OK


def test_predict_x0_null_handle_and_pointers(L):
    _refused(L, L.itsd_sampler_predict_x0(None, 0x1000, None, 1, 0, 1.0, 0.0, 0x2000, None))
    _refused(L, L.itsd_sampler_predict_x0(None, None, None, 1, 0, 1.0, 0.0, None, None))
