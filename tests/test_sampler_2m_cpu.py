"""Host side of the second-order few-step sampler (no GPU): ``schedule.x0_2m_rows`` against a literal evaluation of
DPM-Solver++(2M), its order of accuracy on an analytic model, the refusals of itsd_set_schedule_x0_2m that need no UNet
handle, and the ``sampler: {kind: dpmpp2m}`` config block.

The update, in data prediction, from timestep s = tau[k] to t = tau[k - 1] with alpha = sqrt(abar),
sigma = sqrt(1 - abar), lambda = ln(alpha / sigma), h = lambda_t - lambda_s, r = (lambda_s - lambda_{tau[k+1]}) / h:

    D  = (1 + 1/(2r)) x0_k - (1/(2r)) x0_{k+1}
    x' = (sigma_t / sigma_s) x - alpha_t (e^{-h} - 1) D

Check 1 evaluates that literally in fp64 and compares it with c0 x0_k + cp x0_{k+1} + cx x of the rows, relative 1e-12:
both sides are a handful of fp64 operations on O(1) values (measured over the five schedules: below 1e-13).

Check 3 uses the analytic Gaussian model eps(x, t) = sigma_t x / (abar_t s^2 + sigma_t^2), the exact noise prediction
for data ~ N(0, s^2), whose probability-flow ODE has the closed-form solution
x_t = x_T sqrt((abar_t s^2 + sigma_t^2) / (abar_T s^2 + sigma_T^2)). Measured (fp64): first-order error ratio from
K = 21 to K = 41 1.98; 2M ratio 13.2 at s = 0.5 (3.66 at s = 1.5: theory says 4, hence the bound 3.5); 2M error at
K = 21 a factor 22 below the first-order one."""
import ctypes
import math
import os

import pytest
import torch

from itsd import entry as E
from itsd import runtime as rt
from itsd.schedule import make_schedule, strided_timesteps, x0_2m_rows, x0_form_rows
from test_sampler_x0_cpu import BASE, SCHEDULES, _sched

REL = 1e-12


def _taus(T):
    """Both spacings: strided_timesteps and an explicit, uneven list."""
    K = 4 if T == 12 else 20
    explicit = [0, 3, 4, 9, 11] if T == 12 else [0, 7, 50, 51, 300, 640, 641, T - 2, T - 1]
    return [strided_timesteps(T, K), explicit, strided_timesteps(T, T)[:: max(1, T // 50)]]


# ----------------------------------------------------------------------------- 1. the rows are DPM-Solver++(2M)
@pytest.mark.parametrize("beta_1,beta_T,T", SCHEDULES)
def test_rows_are_the_literal_2m_update(beta_1, beta_T, T):
    ab = [float(v) for v in make_schedule(beta_1, beta_T, T).alphas_bar.double()]
    sched = make_schedule(beta_1, beta_T, T)
    worst = 0.0
    for tau in _taus(T):
        r = x0_2m_rows(sched.alphas_bar, tau)
        K = len(tau)
        assert set(r) == {"a0", "b0", "c0", "cx", "sg", "cp"}
        assert all(v.dtype == torch.float64 and v.shape == (K,) for v in r.values())
        x, x0k, x0p = 1.0, 0.37, -0.81  # the state and two arbitrary x0 estimates
        for k in range(1, K - 1):
            a_s, a_t, a_p = ab[tau[k]], ab[tau[k - 1]], ab[tau[k + 1]]
            alpha_s, sigma_s = math.sqrt(a_s), math.sqrt(1.0 - a_s)
            alpha_t, sigma_t = math.sqrt(a_t), math.sqrt(1.0 - a_t)
            alpha_p, sigma_p = math.sqrt(a_p), math.sqrt(1.0 - a_p)
            lam_s, lam_t, lam_p = math.log(alpha_s / sigma_s), math.log(alpha_t / sigma_t), math.log(alpha_p / sigma_p)
            h = lam_t - lam_s
            rr = (lam_s - lam_p) / h
            D = (1.0 + 1.0 / (2.0 * rr)) * x0k - (1.0 / (2.0 * rr)) * x0p
            want = (sigma_t / sigma_s) * x - alpha_t * math.expm1(-h) * D
            got = float(r["c0"][k]) * x0k + float(r["cp"][k]) * x0p + float(r["cx"][k]) * x
            worst = max(worst, abs(got - want) / abs(want))
            assert float(r["cp"][k]) != 0.0
    print(f"T={T} beta_T={beta_T}: worst relative difference {worst:.3e}")
    assert worst <= REL


# ----------------------------------------------------------------------------- 2. the first-order rows
@pytest.mark.parametrize("beta_1,beta_T,T", SCHEDULES)
def test_end_rows_are_first_order(beta_1, beta_T, T):
    s = make_schedule(beta_1, beta_T, T)
    for tau in _taus(T) + [[T - 1], [3, T - 1]]:
        r, d = x0_2m_rows(s.alphas_bar, tau), x0_form_rows(s.alphas_bar, tau, eta=0.0)
        K = len(tau)
        for k in {0, K - 1}:
            for key in d:
                assert float(r[key][k]) == float(d[key][k]), (tau, k, key)
            assert float(r["cp"][k]) == 0.0
        assert (float(r["c0"][0]), float(r["cx"][0]), float(r["sg"][0])) == (1.0, 0.0, 0.0)
        assert bool((r["sg"] == 0).all())
        for key in ("a0", "b0", "cx"):
            assert torch.equal(r[key], d[key])


# ----------------------------------------------------------------------------- 3. order of accuracy
def _analytic_error(K, second_order, s=0.5):
    sched = make_schedule(1e-4, 0.02, 1000)
    ab = sched.alphas_bar.double()
    tau = [99 + (i * 900) // (K - 1) for i in range(K)]
    rows = x0_2m_rows(ab, tau) if second_order else {**x0_form_rows(ab, tau, 0.0), "cp": torch.zeros(K).double()}
    var = lambda t: float(ab[t]) * s * s + (1.0 - float(ab[t]))  # noqa: E731
    x_T = 1.0
    x, prev = x_T, None
    for k in range(K - 1, 0, -1):
        sig = math.sqrt(1.0 - float(ab[tau[k]]))
        eps = sig * x / var(tau[k])
        x0 = float(rows["a0"][k]) * x - float(rows["b0"][k]) * eps
        x0p = x0 if prev is None else prev
        x = float(rows["c0"][k]) * x0 + float(rows["cp"][k]) * x0p + float(rows["cx"][k]) * x
        prev = x0
    exact = x_T * math.sqrt(var(tau[0]) / var(tau[K - 1]))
    return abs(x - exact) / abs(exact)


def test_order_of_accuracy_on_the_analytic_model():
    e1 = {K: _analytic_error(K, False) for K in (21, 41)}
    e2 = {K: _analytic_error(K, True) for K in (21, 41)}
    e2_wide = {K: _analytic_error(K, True, s=1.5) for K in (21, 41)}
    print(f"first order: {e1}, ratio {e1[21] / e1[41]:.3f}; 2M: {e2}, ratio {e2[21] / e2[41]:.3f}; "
          f"2M at s = 1.5: ratio {e2_wide[21] / e2_wide[41]:.3f}; 2M / first order at K = 21: {e2[21] / e1[21]:.4f}")
    assert 1.7 <= e1[21] / e1[41] <= 2.3
    assert e2[21] / e2[41] >= 3.5
    assert e2_wide[21] / e2_wide[41] >= 3.5
    assert e2[21] < 0.1 * e1[21]


# ----------------------------------------------------------------------------- 4. ABI
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def _cp(vals=(0.25, -0.5, 0.0)):
    return (ctypes.c_float * len(vals))(*vals)


def _refused(L, sc, cp, handle=None):
    rc = L.itsd_set_schedule_x0_2m(handle, None if sc is None else ctypes.byref(sc), cp)
    assert rc == rt.ITSD_ERR_INVALID
    msg = L.itsd_last_error().decode()
    assert "itsd_set_schedule_x0_2m" in msg, msg
    return msg


def test_set_schedule_x0_2m_exported_and_bound(L):
    assert hasattr(ctypes.CDLL(rt.LIB_PATH), "itsd_set_schedule_x0_2m")
    assert "itsd_set_schedule_x0_2m" in rt.EXPORTS
    assert callable(getattr(rt.NativeUNet, "set_schedule_x0_2m"))
    assert rt.RUN_CONTINUE == 8


def test_set_schedule_x0_2m_refusals(L):
    _refused(L, None, _cp())
    for name in ("tau",) + rt.X0_ROW_KEYS:
        assert "null" in _refused(L, _sched(null=name), _cp())
    for K in (0, -3):
        assert "K" in _refused(L, _sched(K=K), _cp())
    for tau in ((2, 2, 8), (5, 2, 8), (-1, 5, 8), (2, 5, 4)):
        assert "tau" in _refused(L, _sched(tau=tau), _cp())
    for c in (2, -1):
        assert "clip_x0" in _refused(L, _sched(clip_x0=c), _cp())
    # its own: a null cp, a cp[k] that is not finite, a top row with a predecessor weight
    assert "null" in _refused(L, _sched(), None)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert "cp[1]" in _refused(L, _sched(), _cp((0.25, bad, 0.0)))
    assert "cp[K - 1]" in _refused(L, _sched(), _cp((0.25, -0.5, 0.125)))
    assert "handle" in _refused(L, _sched(), _cp())  # a valid schedule, no handle: refused last, before any HIP call
    # the first-order call names itself, as before
    assert L.itsd_set_schedule_x0(None, ctypes.byref(_sched())) == rt.ITSD_ERR_INVALID
    assert "itsd_set_schedule_x0:" in L.itsd_last_error().decode()


# ----------------------------------------------------------------------------- config and classes
def test_sampler_block_parsed():
    cfg = {**BASE, "sampler": {"kind": "dpmpp2m", "steps": 20, "clip_x0": True}}
    assert E.sampler_kwargs(cfg, 1000) == {"sampler": "dpmpp2m", "steps": 20, "eta": 0.0, "clip_x0": True}
    assert E.sampler_kwargs({**BASE, "sampler": {"kind": "DPMPP2M", "eta": 0.0}}, 12) == \
        {"sampler": "dpmpp2m", "steps": None, "eta": 0.0, "clip_x0": False}
    cfg = E.load_config(dict(BASE), ["sampler.kind=dpmpp2m", "sampler.steps=7"])
    assert E.sampler_kwargs(cfg, 12) == {"sampler": "dpmpp2m", "steps": 7, "eta": 0.0, "clip_x0": False}


@pytest.mark.parametrize("block,key", [
    ({"kind": "dpmpp2m", "eta": 0.5}, "sampler.eta"),
    ({"kind": "dpmpp2m", "eta": 1.0}, "sampler.eta"),
    ({"kind": "dpmpp2m", "steps": 13}, "sampler.steps"),
    ({"kind": "dpmpp2m", "clip_x0": 1}, "sampler.clip_x0"),
    ({"kind": "dpmpp3m"}, "sampler.kind"),
])
def test_sampler_block_refusals(block, key):
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        E.sampler_kwargs({**BASE, "sampler": block}, 12)


def test_particle_search_names_dpmpp2m():
    cfg = {**BASE, "sampler": {"kind": "dpmpp2m", "steps": 6}, "search": {"algorithm": "particle"}}
    with pytest.raises(ValueError, match=r"sampler\.(kind|eta).*dpmpp2m"):
        E.particle_args(cfg, 12)


def test_sampler_classes_validate_without_a_device():
    from itsd.diffusion import CondGaussianDiffusionSampler, GaussianDiffusionSampler

    s = GaussianDiffusionSampler(None, 1e-4, 0.02, 12, sampler="dpmpp2m", steps=4, clip_x0=True)
    assert s.n_steps == 4 and s.tau == [2, 5, 8, 11] and s.T == 12 and s.x0_form and s.eta == 0.0
    assert torch.equal(s.abar_rows, s.sched.alphas_bar[torch.tensor([2, 5, 8, 11])])
    assert set(s.rows) == {"a0", "b0", "c0", "cx", "sg", "cp"}
    want = x0_2m_rows(s.sched.alphas_bar, [2, 5, 8, 11])
    assert all(torch.equal(s.rows[k], want[k]) for k in want)
    d = CondGaussianDiffusionSampler(None, 1e-4, 0.028, 12, w=1.8, sampler="dpmpp2m", steps=[0, 7, 11])
    assert d.tau == [0, 7, 11] and d.sampler == "dpmpp2m"
    assert not GaussianDiffusionSampler(None, 1e-4, 0.02, 12).x0_form
    assert GaussianDiffusionSampler(None, 1e-4, 0.02, 12, sampler="ddim").x0_form
    for kw in (dict(eta=0.5), dict(eta=1.0), dict(steps=13), dict(steps=0)):
        with pytest.raises(ValueError):
            GaussianDiffusionSampler(None, 1e-4, 0.02, 12, sampler="dpmpp2m", **kw)
    with pytest.raises(ValueError, match="reference"):
        s.denoise_fn(reference_rng=True)
    with pytest.raises(ValueError, match="reference"):
        s.reference_noise((1, 3, 8, 8))
