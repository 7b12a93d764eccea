"""Host-side contract of the op-program probe (itsd_unet_op_info / _act_info / _read / _poison): the four calls are
exported and bound, the ctypes mirrors of their structs have the header's layout, and every call refuses a null
handle or a null output with ITSD_ERR_INVALID and a message before any device call (so this runs without a GPU).
The range and byte-count checks need a handle: tests/test_gpu_ops.py::test_probe_refuses_bad_arguments."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from itsd import runtime as rt

PROBE = ("itsd_unet_op_info", "itsd_unet_act_info", "itsd_unet_read", "itsd_unet_poison")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def _refused(L, rc):
    assert rc == rt.ITSD_ERR_INVALID
    assert L.itsd_last_error().decode()  # a message, not an empty string


def test_symbols_exported_and_bound(L):
    lib = ctypes.CDLL(rt.LIB_PATH)
    for name in PROBE:
        assert hasattr(lib, name), f"missing export {name}"
        assert name in rt.EXPORTS


def _header_struct_fields(name):
    src = open(os.path.join(ROOT, "include", "itsd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            m = re.match(r"(\w+)\[(\d+)\]", nm)
            out.append((m.group(1), typ, int(m.group(2))) if m else (nm, typ, 0))
    return out


@pytest.mark.parametrize("cname,mirror", [("itsd_op_info", rt.OpInfo), ("itsd_act_info", rt.ActInfo)])
def test_struct_mirrors_match_header(cname, mirror):
    want = _header_struct_fields(cname)
    got = list(mirror._fields_)
    assert [w[0] for w in want] == [g[0] for g in got]
    size = 0
    for (nm, typ, arr), (_, ct) in zip(want, got):
        if typ == "int32_t":
            assert ct is ctypes.c_int32, nm
            size += 4
        else:
            assert typ == "char" and ctypes.sizeof(ct) == arr, nm
            size += arr
    assert ctypes.sizeof(mirror) == size  # int32 fields then a char array: no padding


def test_null_handle_and_outputs(L):
    oi, ai = rt.OpInfo(), rt.ActInfo()
    _refused(L, L.itsd_unet_op_info(None, rt.PASS_FORWARD, 1, 1, ctypes.byref(oi)))
    _refused(L, L.itsd_unet_op_info(None, rt.PASS_STEP, 1, 1, None))
    _refused(L, L.itsd_unet_act_info(None, 0, ctypes.byref(ai)))
    _refused(L, L.itsd_unet_act_info(None, rt.ACT_PROJ, ctypes.byref(ai)))
    _refused(L, L.itsd_unet_act_info(None, 0, None))
    for what in (rt.READ_ACT, rt.READ_STATS, rt.READ_COEF, rt.READ_PROJ, 9, -1):
        _refused(L, L.itsd_unet_read(None, what, 0, 1, 0x10000, 64, None))
        _refused(L, L.itsd_unet_read(None, what, 0, 1, None, 64, None))
    _refused(L, L.itsd_unet_poison(None, None))


def test_enumerators_match_header():
    src = open(os.path.join(ROOT, "include", "itsd.h")).read()
    for name, val in (("ITSD_OP_GN", rt.OP_GN), ("ITSD_OP_CONV", rt.OP_CONV), ("ITSD_OP_ATTN", rt.OP_ATTN),
                      ("ITSD_OP_GNCOEF", rt.OP_GNCOEF), ("ITSD_OP_ATTNBLOCK", rt.OP_ATTNBLOCK),
                      ("ITSD_OP_HEAD", rt.OP_HEAD), ("ITSD_OP_TAIL", rt.OP_TAIL), ("ITSD_TAG_QKV", rt.TAG_QKV),
                      ("ITSD_TAG_DOWN_MERGE", rt.TAG_DOWN_MERGE), ("ITSD_TAG_ATTN_S1", rt.TAG_ATTN_S1),
                      ("ITSD_TAG_CONVT", rt.TAG_CONVT), ("ITSD_TAG_ATTNBLOCK", rt.TAG_ATTNBLOCK),
                      ("ITSD_PASS_FORWARD", rt.PASS_FORWARD), ("ITSD_PASS_STEP", rt.PASS_STEP),
                      ("ITSD_READ_ACT", rt.READ_ACT), ("ITSD_READ_STATS", rt.READ_STATS),
                      ("ITSD_READ_COEF", rt.READ_COEF), ("ITSD_READ_PROJ", rt.READ_PROJ)):
        assert re.search(name + r" = " + str(val) + r"\b", src), name
    assert re.search(r"#define ITSD_ACT_PROJ \(" + str(rt.ACT_PROJ) + r"\)", src)
    # ConvKernel's order in csrc/common.h is what itsd_op_info::kernel counts in
    pkg = os.path.dirname(rt.__file__)
    enum = re.search(r"enum class ConvKernel \{(.*?)\};", open(os.path.join(pkg, "csrc", "common.h")).read(), re.S).group(1)
    names = re.findall(r"^\s*(\w+),", enum, re.M)
    assert tuple(names) == rt.CONV_KERNELS
