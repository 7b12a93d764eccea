"""GPU tests of the sampler step every tail kernel ends in, at a step t > 0: the noise branch (injected and Philox),
the clip and the NaN flag, for each of the six forms the launcher can select (TAIL_CASES of test_gpu_path_branch.py,
whose docstring names the kernel each case runs; test_x0_at_t0_is_the_samplers_last_step there covers t = 0 only).

One step t = 5 of T = 12 (t_begin = t_end = t), run several times on the same input. Every check is bit equality:
each compares two runs of the same program on the same batch, which differ only in the step epilogue's operands,
and the epilogue is  mean = c1 x - c2 eps;  x' = mean + sv z  with contraction off -- a separate fp32 multiply and
add, which torch repeats exactly from the zero-noise step (x' = mean) and the schedule's fp32 sqrt_var[t]."""
import pytest
import torch

from itsd import runtime as rt
from test_gpu_path_branch import DEV, TAIL_CASES, T, _sampler, _x

pytestmark = pytest.mark.gpu

STEP = 5  # 0 < STEP < T - 1
SEED = 0x5EED


def _steps(case):
    """The runs of one tail form (one sampler, made inside the io_mfma window) that the checks compare."""
    a, precision, io_mfma, n = TAIL_CASES[case]
    t = STEP
    rt.set_option("io_mfma", io_mfma)
    try:
        smp = _sampler(a, precision)
        x = _x(n, a.img_size, seed=3)
        lab = torch.tensor([3, 7], dtype=torch.int32, device=DEV)[:n] if a.cfg else None
        sv = smp.sched.sqrt_var_f32[t].to(DEV)
        assert 0 < t < T - 1 and sv.dtype == torch.float32 and float(sv) > 0.0
        shape = (t + 1,) + tuple(x.shape)
        Z = torch.randn(shape, generator=torch.Generator().manual_seed(17)).to(DEV)
        zeros = torch.zeros(shape, device=DEV)
        per = x[0].numel()

        def run(tt=t, **kw):
            return smp.run(x.clone(), t_begin=tt, t_end=tt, labels=lab, **kw)

        r = {"n": n, "per": per, "sv": sv, "Z": Z, "x": x}
        r["mean"] = run(noise=zeros, clip=False)
        r["mean_again"] = run(noise=zeros, clip=False)
        r["injected"] = run(noise=Z, clip=False)
        r["philox"] = run(seed=SEED, clip=False)
        r["philox_off"] = run(seed=SEED, noise_offset=3 * per, clip=False)
        r["clipped"] = run(noise=Z, clip=True)
        r["t0_Z"] = run(0, noise=Z, clip=False)
        r["t0_zeros"] = run(0, noise=zeros, clip=False)
        # the NaN flag: one NaN in the draw of step t; one in the draw of step t + 1, which is not run
        bad = Z.clone()
        bad[t, n - 1, 1, 5, 7] = float("nan")
        r["nan_raised"] = []
        for graph in (True, False):
            with pytest.raises(AssertionError, match="nan in tensor"):
                run(noise=bad, clip=False, graph=graph)
            r["nan_raised"].append(graph)
        r["after_nan"] = run(noise=Z, clip=False)  # run_begin_kernel resets the flag
        other = torch.cat([Z, torch.zeros_like(Z[:1])])
        other[t + 1, n - 1, 1, 5, 7] = float("nan")
        r["nan_elsewhere"] = run(noise=other, clip=False)
    finally:
        rt.set_option("io_mfma", 1)
    return r


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_step_noise_clip_and_nan_flag(case):
    r = _steps(case)
    t, n, per, sv, Z, m = STEP, r["n"], r["per"], r["sv"], r["Z"], r["mean"]
    assert torch.isfinite(m).all() and not torch.equal(m, r["x"])
    assert torch.equal(m, r["mean_again"]), f"{case}: two runs of one step differ"
    # 1. injected noise
    want = m + sv * Z[t]
    assert torch.equal(r["injected"], want), f"{case}: max|d| {(r['injected'] - want).abs().max().item():.3e}"
    assert not torch.equal(want, m)
    # 2. Philox: the draw of (seed, stream t) for element o of candidate offset 0, and of offset k
    for key, k in (("philox", 0), ("philox_off", 3)):
        z = rt.noise(torch.empty_like(m), n, SEED, t, cand_offset=k)
        want_p = m + sv * z
        assert torch.equal(r[key], want_p), f"{case} {key}: max|d| {(r[key] - want_p).abs().max().item():.3e}"
    assert not torch.equal(r["philox"], r["philox_off"])
    # 3. the clip (some element is outside [-1, 1], so the clip is seen)
    assert float(want.abs().max()) > 1.0
    assert torch.equal(r["clipped"], want.clamp(-1.0, 1.0)), f"{case}: clip"
    # 4. no draw at t = 0
    assert torch.equal(r["t0_Z"], r["t0_zeros"]), f"{case}: step 0 used its noise"
    # 5. the NaN flag
    assert r["nan_raised"] == [True, False]
    assert torch.equal(r["after_nan"], want), f"{case}: the run after a flagged one"
    assert torch.equal(r["nan_elsewhere"], want), f"{case}: a NaN in a draw that is not used"
