"""Host side of the few-step sampler (no GPU): the row -> timestep spacing, the x0-form row coefficients against the
reference-pinned schedule, the refusals of itsd_set_schedule_x0 that need no UNet handle, and the ``sampler:`` config
block.

Row identities. With every timestep a row (tau = range(T)) and eta = 1 the x0-form step
    x' = c0 (a0 x - b0 eps) + cx x + sg z
is the ancestral step coeff1 x - coeff2 eps + sqrt(posterior_var) z, so c0 a0 + cx = coeff1, c0 b0 = coeff2 and
sg^2 = posterior_var (k >= 1). Both sides are fp64; the bound is relative 1e-10. The largest value measured over
(1e-4, 0.02, T = 12 / 1000 / 3000) and (1e-4, 0.028, T = 12 / 1000) is 3.2e-13 (c0 b0 against coeff2 at T = 1000,
beta_T = 0.028: 1 - abar cancels near t = 0), about 300 x inside the bound."""
import ctypes
import os

import pytest
import torch

from itsd import entry as E
from itsd import runtime as rt
from itsd.schedule import check_timesteps, make_schedule, strided_timesteps, x0_coeffs, x0_form_rows

REL = 1e-10
SCHEDULES = [(1e-4, 0.02, 12), (1e-4, 0.02, 1000), (1e-4, 0.02, 3000), (1e-4, 0.028, 12), (1e-4, 0.028, 1000)]


# ----------------------------------------------------------------------------- spacing
@pytest.mark.parametrize("T", [12, 1000, 3000])
def test_strided_timesteps(T):
    for K in (1, 2, 4, 5, 7, T // 2, T):
        tau = strided_timesteps(T, K)
        assert len(tau) == K and tau[-1] == T - 1 and tau[0] >= 0
        assert all(b > a for a, b in zip(tau, tau[1:])), f"T={T} K={K}: not strictly increasing"
        assert tau == [((k + 1) * T) // K - 1 for k in range(K)]
    assert strided_timesteps(T, T) == list(range(T))
    for K in (0, -1, T + 1):
        with pytest.raises(ValueError, match="steps"):
            strided_timesteps(T, K)


def test_strided_timesteps_T12_K4():
    assert strided_timesteps(12, 4) == [2, 5, 8, 11]


def test_explicit_timesteps():
    assert check_timesteps([0, 3, 11], 12) == [0, 3, 11]
    for bad in ([], [3, 3], [5, 2], [-1, 4], [0, 12]):
        with pytest.raises(ValueError, match="timesteps"):
            check_timesteps(bad, 12)


# ----------------------------------------------------------------------------- rows
def _rel(got, want):
    return float(((got - want).abs() / want.abs()).max())


@pytest.mark.parametrize("beta_1,beta_T,T", SCHEDULES)
def test_rows_reproduce_the_ancestral_schedule(beta_1, beta_T, T):
    s = make_schedule(beta_1, beta_T, T)
    r = x0_form_rows(s.alphas_bar, range(T), eta=1.0)
    assert all(v.dtype == torch.float64 and v.shape == (T,) for v in r.values())
    figures = {"coeff1": _rel(r["c0"] * r["a0"] + r["cx"], s.coeff1), "coeff2": _rel(r["c0"] * r["b0"], s.coeff2),
               "var": _rel(r["sg"][1:] ** 2, s.posterior_var[1:])}
    print(f"T={T} beta_T={beta_T}: {figures}")
    assert all(v <= REL for v in figures.values()), figures
    assert (float(r["c0"][0]), float(r["cx"][0]), float(r["sg"][0])) == (1.0, 0.0, 0.0)
    for k in (0, T // 2, T - 1):  # a0, b0 are x0_coeffs' own values
        assert (float(r["a0"][k]), float(r["b0"][k])) == x0_coeffs(s.alphas_bar, k)


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_rows_of_a_strided_schedule(eta):
    s = make_schedule(1e-4, 0.02, 1000)
    tau = strided_timesteps(1000, 50)
    r = x0_form_rows(s.alphas_bar, tau, eta)
    assert (float(r["c0"][0]), float(r["cx"][0]), float(r["sg"][0])) == (1.0, 0.0, 0.0)
    if eta == 0.0:
        assert bool((r["sg"] == 0).all())
    else:
        assert bool((r["sg"][1:] > 0).all())
    # the step maps (x0, eps) at abar[tau[k]] to the same pair at abar[tau[k-1]]: c0 + cx sqrt(a) = sqrt(p) and
    # cx^2 (1 - a) + sg^2 = 1 - p
    ab = s.alphas_bar[torch.tensor(tau)]
    p = torch.cat([torch.ones(1, dtype=torch.float64), ab[:-1]])
    assert _rel(r["c0"] + r["cx"] * ab.sqrt(), p.sqrt()) <= REL
    assert float((r["cx"] ** 2 * (1 - ab) + r["sg"] ** 2 - (1 - p)).abs().max()) <= REL
    assert bool((r["cx"] < 1).all()) and bool((r["cx"] >= 0).all())


# ----------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def _sched(K=3, tau=(2, 5, 8), clip_x0=1, null=None):
    keep = [(ctypes.c_int32 * len(tau))(*tau)] + [(ctypes.c_float * max(1, len(tau)))() for _ in rt.X0_ROW_KEYS]
    sc = rt.X0Schedule()
    sc.K = K
    sc.tau = keep[0]
    for k, buf in zip(rt.X0_ROW_KEYS, keep[1:]):
        setattr(sc, k, buf)
    if null == "tau":
        sc.tau = ctypes.POINTER(ctypes.c_int32)()
    elif null:
        setattr(sc, null, ctypes.POINTER(ctypes.c_float)())
    sc.clip_x0 = clip_x0
    sc.w = 0.0
    sc._keep = keep
    return sc


def _refused(L, sc, handle=None):
    rc = L.itsd_set_schedule_x0(handle, None if sc is None else ctypes.byref(sc))
    assert rc == rt.ITSD_ERR_INVALID
    assert L.itsd_last_error().decode()
    return L.itsd_last_error().decode()


def test_set_schedule_x0_exported_and_bound(L):
    assert hasattr(ctypes.CDLL(rt.LIB_PATH), "itsd_set_schedule_x0")
    assert "itsd_set_schedule_x0" in rt.EXPORTS
    assert callable(getattr(rt.NativeUNet, "set_schedule_x0"))


def test_set_schedule_x0_refusals(L):
    _refused(L, None)
    for name in ("tau",) + rt.X0_ROW_KEYS:
        assert "null" in _refused(L, _sched(null=name))
    for K in (0, -3):
        assert "K" in _refused(L, _sched(K=K))
    for tau in ((2, 2, 8), (5, 2, 8), (-1, 5, 8), (2, 5, 4)):
        assert "tau" in _refused(L, _sched(tau=tau))
    for c in (2, -1):
        assert "clip_x0" in _refused(L, _sched(clip_x0=c))
    assert "handle" in _refused(L, _sched())  # a valid schedule, no handle: refused last, still before any HIP call


# ----------------------------------------------------------------------------- config
BASE = {"T": 1000, "beta_1": 1e-4, "beta_T": 0.02}


def test_sampler_block_parsed():
    assert E.sampler_kwargs(dict(BASE), 1000) == {}
    assert E.sampler_kwargs({**BASE, "sampler": {"kind": "ddpm"}}, 1000) == {}
    cfg = {**BASE, "sampler": {"kind": "ddim", "steps": 50, "eta": 0.0, "clip_x0": True}}
    assert E.sampler_kwargs(cfg, 1000) == {"sampler": "ddim", "steps": 50, "eta": 0.0, "clip_x0": True}
    assert E.sampler_kwargs({**BASE, "sampler": {"kind": "ddim"}}, 12) == \
        {"sampler": "ddim", "steps": None, "eta": 0.0, "clip_x0": False}
    # Hydra-style overrides, as for search.*
    cfg = E.load_config(cfg, ["sampler.steps=20", "sampler.eta=0.5", "sampler.clip_x0=false"])
    assert E.sampler_kwargs(cfg, 1000) == {"sampler": "ddim", "steps": 20, "eta": 0.5, "clip_x0": False}
    cfg = E.load_config(dict(BASE), ["sampler.kind=ddim", "sampler.steps=7"])
    assert E.sampler_kwargs(cfg, 12)["steps"] == 7


@pytest.mark.parametrize("block,key", [
    ({"kind": "plms"}, "sampler.kind"),
    ({"kind": "ddim", "steps": 0}, "sampler.steps"),
    ({"kind": "ddim", "steps": 13}, "sampler.steps"),     # > inference T = 12
    ({"kind": "ddim", "steps": 2.5}, "sampler.steps"),
    ({"kind": "ddim", "eta": -0.1}, "sampler.eta"),
    ({"kind": "ddim", "eta": 1.5}, "sampler.eta"),
    ({"kind": "ddim", "eta": "big"}, "sampler.eta"),
    ({"kind": "ddim", "clip_x0": 1}, "sampler.clip_x0"),
    ({"kind": "ddim", "clip_x0": "yes"}, "sampler.clip_x0"),
])
def test_sampler_block_refusals(block, key):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        E.sampler_kwargs({**BASE, "sampler": block}, 12)


def test_sampler_classes_validate_without_a_device():
    from itsd.diffusion import CondGaussianDiffusionSampler, GaussianDiffusionSampler

    s = GaussianDiffusionSampler(None, 1e-4, 0.02, 12, sampler="ddim", steps=4, eta=0.5, clip_x0=True)
    assert s.n_steps == 4 and s.tau == [2, 5, 8, 11] and s.T == 12
    assert torch.equal(s.abar_rows, s.sched.alphas_bar[torch.tensor([2, 5, 8, 11])])
    d = CondGaussianDiffusionSampler(None, 1e-4, 0.028, 12, w=1.8)
    assert d.n_steps == 12 and d.abar_rows is d.sched.alphas_bar and d.sampler == "ddpm"
    assert GaussianDiffusionSampler(None, 1e-4, 0.02, 12, sampler="ddim").n_steps == 12
    assert GaussianDiffusionSampler(None, 1e-4, 0.02, 12, sampler="ddim", steps=[0, 7, 11]).tau == [0, 7, 11]
    for kw in (dict(sampler="euler"), dict(sampler="ddim", steps=13), dict(sampler="ddim", eta=2.0), dict(steps=4)):
        with pytest.raises(ValueError):
            GaussianDiffusionSampler(None, 1e-4, 0.02, 12, **kw)
    with pytest.raises(ValueError, match="reference"):
        s.denoise_fn(reference_rng=True)
    with pytest.raises(ValueError, match="reference"):
        s.reference_noise((1, 3, 8, 8))
