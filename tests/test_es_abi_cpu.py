"""Host-side contract of the ES gradient's entry points -- itsd_es_workspace_bytes, itsd_es_candidates, itsd_es_step:
they are exported and bound, and every invalid-argument case is refused with ITSD_ERR_INVALID and a message before any
device call (so this runs without a GPU). Pointers are plain integers: a refused call never dereferences one."""
import ctypes
import math
import os

import pytest

from itsd import runtime as rt

NAMES = ("itsd_es_workspace_bytes", "itsd_es_candidates", "itsd_es_step")
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def _refused(L, rc):
    assert rc == rt.ITSD_ERR_INVALID
    assert L.itsd_last_error().decode()  # a message, not an empty string


def _adam(**kw):
    f = dict(beta1=0.9, omb1=0.1, beta2=0.999, omb2=0.001, c1=0.1, c2=31.6, eps=1e-8)
    f.update(kw)
    return rt.AdamStep(*[f[k] for k, _ in rt.AdamStep._fields_])


def _cand(L, out=0x10000, pivot=0x20000, n_cand=2, per=4, sigma=0.1, cand_offset=0):
    return L.itsd_es_candidates(out, pivot, n_cand, per, sigma, 1, 2, cand_offset, None)


# five disjoint, 16-byte aligned ranges, 1 MiB apart
_BASE = dict(theta=0x100000, m=0x200000, v=0x300000, grad_out=0x400000, ws=0x500000)


def _step(L, n_pairs=3, per=8, adam="default", w=0x600000, gnorm2=0x700000, **ptr):
    p = dict(_BASE)
    p.update(ptr)
    a = _adam() if adam == "default" else adam
    return L.itsd_es_step(p["theta"], p["m"], p["v"], w, n_pairs, per, 1, 2, None if a is None else ctypes.byref(a),
                          p["grad_out"], gnorm2, p["ws"], None)


def test_symbols_exported_and_bound(L):
    lib = ctypes.CDLL(rt.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"missing export {name}"
        assert name in rt.EXPORTS + rt.EXPORTS_I64
    assert rt.EXPORTS_I64 == ("itsd_es_workspace_bytes",)  # (an int64_t size, bound beside the status-returning calls)
    assert L.itsd_es_workspace_bytes.restype is ctypes.c_int64
    assert [k for k, _ in rt.AdamStep._fields_] == ["beta1", "omb1", "beta2", "omb2", "c1", "c2", "eps"]
    assert ctypes.sizeof(rt.AdamStep) == 28
    for fn in ("es_candidates", "es_step", "es_workspace_bytes", "adam_coeffs"):
        assert callable(getattr(rt, fn))


def test_workspace_bytes(L):
    ws = L.itsd_es_workspace_bytes
    for bad in ((0, 16), (-1, 16), (4, 0), (4, -8)):
        assert ws(*bad) <= 0
    with pytest.raises(rt.ItsdError):
        rt.es_workspace_bytes(0, 16)
    pers = (1, 3, 75, 1024, 1027, 3072, 49152, 1 << 22)
    pairs = (1, 2, 15, 16, 17, 32, 33, 257, 512, 4096)
    for per in pers:
        sizes = [ws(m, per) for m in pairs]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (per, sizes)  # monotone in n_pairs
        for m, s in zip(pairs, sizes):
            assert s >= math.ceil(m / 16) * per * 4  # at least the slice sums
            assert rt.es_workspace_bytes(m, per) == s
    for m in pairs:
        sizes = [ws(m, per) for per in pers]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (m, sizes)    # monotone in per_cand
    assert ws(512, 49152) < 2 * 32 * 49152 * 4  # (and not wastefully more)


def test_candidates_refusals(L):
    _refused(L, _cand(L, out=None))
    _refused(L, _cand(L, pivot=None))
    _refused(L, _cand(L, n_cand=-1))
    _refused(L, _cand(L, per=0))
    _refused(L, _cand(L, per=-4))
    _refused(L, _cand(L, cand_offset=-1))
    for sigma in (0.0, -0.1, INF, -INF, NAN):
        _refused(L, _cand(L, sigma=sigma))


def test_candidates_zero_rows_is_a_noop(L):
    assert _cand(L, n_cand=0) == rt.ITSD_OK  # (nothing is launched: out / pivot above are not device memory)
    _refused(L, _cand(L, n_cand=0, sigma=0.0))  # the arguments are still checked


def test_step_null_pointers(L):
    for name in ("theta", "m", "v", "ws"):
        _refused(L, _step(L, **{name: None}))
    _refused(L, _step(L, w=None))
    _refused(L, _step(L, gnorm2=None))
    _refused(L, _step(L, adam=None))


def test_step_sizes(L):
    _refused(L, _step(L, n_pairs=0))
    _refused(L, _step(L, n_pairs=-3))
    _refused(L, _step(L, per=0))
    _refused(L, _step(L, per=-8))


def test_step_adam_fields(L):
    for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=1.5), dict(beta2=1.0), dict(beta2=-1e-3),
               dict(eps=0.0), dict(eps=-1e-8)):
        _refused(L, _step(L, adam=_adam(**kw)))
    for k, _ in rt.AdamStep._fields_:
        for bad in (INF, -INF, NAN):
            _refused(L, _step(L, adam=_adam(**{k: bad})))


def test_step_overlapping_ranges(L):
    per, n_pairs = 8, 3  # theta / m / v / grad_out: 32 bytes each
    ws_bytes = L.itsd_es_workspace_bytes(n_pairs, per)
    names = list(_BASE)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            size_a = ws_bytes if a == "ws" else per * 4
            size_b = ws_bytes if b == "ws" else per * 4
            # b starts inside a, at a's last 16-byte step; b ends inside a; the two coincide
            for pb in (_BASE[a], _BASE[a] + (size_a - 1) // 16 * 16, _BASE[a] - (size_b - 1) // 16 * 16):
                _refused(L, _step(L, n_pairs=n_pairs, per=per, **{b: pb}))
                assert a in L.itsd_last_error().decode() and b in L.itsd_last_error().decode()


def test_step_grad_out_may_be_null(L):
    """grad_out is optional: a null one is not an argument error (checked through a call another argument refuses, so
    nothing is launched: the message must name that other argument)."""
    _refused(L, _step(L, grad_out=None, adam=_adam(eps=0.0)))
    assert "eps" in L.itsd_last_error().decode()
