"""GPU tests of the few-step sampler: the x0-form step epilogue of every tail kernel (TailArgs::step_mode 3), the row
schedule behind it (itsd_set_schedule_x0), and the searches in units of rows. T = 12 and K = 4 rows (tau = 2, 5, 8, 11)
unless a check says otherwise; the six tail forms are TAIL_CASES of test_gpu_path_branch.py, whose docstring names the
kernel each one runs.

The step is, in fp32 with contraction off,
    x0 = a0 x - b0 e  (clipped iff clip_x0);   m = (c0 x0) + (cx x);   x' = sg != 0 ? m + sg z : m
so whatever compares two runs of one program that differ only in epilogue operands is bit equality, and torch repeats
the epilogue exactly from predict_x0 (the same a0 x - b0 e, clipped) and the fp32 casts of the row.

One check is not bit equality -- the unclipped step at K = T, eta = 1 against the ancestral step (check 2). There
c0 a0 + cx = coeff1 and c0 b0 = coeff2 hold in fp64 (test_sampler_x0_cpu.py), but the device rounds five constants
instead of two and associates differently. With u = 2^-24 (half an ulp), the x0-form side computes
    fl(fl(c0 fl(fl(a0 x) - fl(b0 e))) + fl(cx x))
whose error against the exact c0 (a0 x - b0 e) + cx x is, to first order, at most
    |c0| (|a0 x| + |b0 e|) (u_a0|b0 + u_mul + u_sub + u_c0 + u_mul + u_add) + |cx x| (u_cx + u_mul + u_add)
    <= 6u |c0| (|a0 x| + |b0 e|) + 3u |cx x|,
and the ancestral side fl(fl(c1 x) - fl(c2 e)) errs by at most 3u (|coeff1 x| + |coeff2 e|) (constant, multiply,
subtract). The sum is below 8u = 2^-21 times (|c0| (|a0 x| + |b0 e|) + |cx x| + |coeff1 x| + |coeff2 e|): the bound
asserted, the form of the t = 0 bound of test_gpu_path_branch.py. e enters the magnitude only (the forward API's eps,
guided in torch for CFG).

The whole loop against the fp64 oracle (check 7) uses DESIGN section 4's own bounds for trajectories of T <= 20 steps:
fp32 max-abs <= 2e-3, bf16 relative L2 <= 3e-2."""
import dataclasses

import pytest
import torch

from itsd import runtime as rt
from itsd.arch import ARCH_TINY
from itsd.schedule import x0_coeffs
from itsd.search import SearchEngine
from itsd.verifier import OracleVerifier
from itsd.weights import synthetic_state_dict
from oracle import ref_cpu as R
from test_gpu_path_branch import DEV, MASK62, TAIL_CASES, TINY_CFG, T, _sampler, _x

pytestmark = pytest.mark.gpu

K = 4
TAU = [2, 5, 8, 11]
SEED = 0x5EED
SHAPE = (1, 3, 32, 32)


def _ddim(smp, steps=K, eta=0.0, clip_x0=False):
    """A few-step sampler over the net (and the schedule) of the ancestral sampler smp."""
    return type(smp)(smp.model, smp.sched.beta_1, smp.sched.beta_T, T, w=smp.w, sampler="ddim", steps=steps, eta=eta,
                     clip_x0=clip_x0)


def _row(smp, k):
    """The fp32 casts of row k, as device scalars."""
    return {key: v[k].float().to(DEV) for key, v in smp.rows.items()}


def _labels(a, n):
    return torch.tensor([3, 7], dtype=torch.int32, device=DEV)[:n] if a.cfg else None


def _eps(smp, x, t, lab):
    if lab is None:
        return smp.model(x, t).double()
    return (1.0 + smp.w) * smp.model(x, t, lab).double() - smp.w * smp.model(x, t, torch.zeros_like(lab)).double()


def _forms(case):
    """Every run checks 1-4 compare, for one tail form (the samplers are made inside its io_mfma window)."""
    a, precision, io_mfma, n = TAIL_CASES[case]
    rt.set_option("io_mfma", io_mfma)
    try:
        base = _sampler(a, precision)
        x, lab = _x(n, a.img_size, seed=3), _labels(a, n)
        per = x[0].numel()
        Z = torch.randn((K,) + tuple(x.shape), generator=torch.Generator().manual_seed(17)).to(DEV)
        nan = torch.full_like(Z, float("nan"))
        r = {"x": x, "Z": Z, "n": n, "per": per}
        # 1. the clipped step with injected noise
        s = _ddim(base, eta=0.5, clip_x0=True)
        assert s.tau == TAU and s._native(n).query("sched_form") == 1 and s._native(n).query("T_sched") == K
        r["row"] = _row(s, 2)
        r["x0"] = s.predict_x0(x, 2, labels=lab)
        r["step"] = s.run(x.clone(), t_begin=2, t_end=2, labels=lab, noise=Z, clip=False)
        # 3. no draw where sg == 0
        det = _ddim(base, eta=0.0, clip_x0=True)
        r["det_nan"] = det.run(x.clone(), labels=lab, noise=nan)
        r["det_zero"] = det.run(x.clone(), labels=lab, noise=torch.zeros_like(Z))
        # 4. Philox, and row 0 of an eta = 1 sampler
        st = _ddim(base, eta=1.0, clip_x0=True)
        r["sg2"] = float(st.rows["sg"][2])
        r["philox"] = [st.run(x.clone(), t_begin=2, t_end=2, labels=lab, seed=SEED, noise_offset=k * per, clip=False)
                       for k in (0, 3)]
        r["injected"] = []
        for k in (0, 3):
            z = torch.zeros_like(Z)
            rt.noise(z[2], n, SEED, 2, cand_offset=k)
            r["injected"].append(st.run(x.clone(), t_begin=2, t_end=2, labels=lab, noise=z, clip=False))
        r["row0_nan"] = st.run(x.clone(), t_begin=0, t_end=0, labels=lab, noise=nan, clip=False)
        r["row0_zero"] = st.run(x.clone(), t_begin=0, t_end=0, labels=lab, noise=torch.zeros_like(Z), clip=False)
        # 2. K = T, eta = 1: the ancestral mean
        zeros = torch.zeros((6,) + tuple(x.shape), device=DEV)
        full = _ddim(base, steps=T, eta=1.0, clip_x0=False)
        fullc = _ddim(base, steps=T, eta=1.0, clip_x0=True)
        r["full_row"] = {k: float(v[5].float()) for k, v in full.rows.items()}
        r["full"] = full.run(x.clone(), t_begin=5, t_end=5, labels=lab, noise=zeros, clip=False)
        r["full_clipped"] = fullc.run(x.clone(), t_begin=5, t_end=5, labels=lab, noise=zeros, clip=False)
        r["full_x0"] = fullc.predict_x0(x, 5, labels=lab)
        r["ddpm"] = base.run(x.clone(), t_begin=5, t_end=5, labels=lab, noise=zeros, clip=False)
        r["c12"] = (float(base.sched.coeff1_f32[5]), float(base.sched.coeff2_f32[5]))
        r["eps5"] = _eps(base, x, 5, lab)
    finally:
        rt.set_option("io_mfma", 1)
    return r


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_x0_form_step_every_tail_form(case):
    r = _forms(case)
    x, Z = r["x"], r["Z"]
    # 1. clipped step, bit-exact
    row, x0 = r["row"], r["x0"]
    rail = float((x0.abs() == 1.0).float().mean())
    print(f"{case}: share of x0 on a rail {rail:.3f}")
    assert 0.01 <= rail <= 0.99, f"{case}: {rail:.3f} of x0 on a rail: one branch of the clip is not seen"
    assert float(row["sg"]) > 0.0
    want = (row["c0"] * x0 + row["cx"] * x) + row["sg"] * Z[2]
    assert torch.equal(r["step"], want), f"{case}: max|d| {(r['step'] - want).abs().max().item():.3e}"
    # 2. unclipped, every timestep a row, eta = 1: the ancestral mean within rounding
    f, (c1, c2), xd, e = r["full_row"], r["c12"], x.double(), r["eps5"]
    bound = 2.0 ** -21 * (abs(f["c0"]) * ((f["a0"] * xd).abs() + (f["b0"] * e).abs()) + (f["cx"] * xd).abs()
                          + (c1 * xd).abs() + (c2 * e).abs())
    d = (r["full"].double() - r["ddpm"].double()).abs()
    print(f"{case}: x0-form vs ancestral max|d| {d.max().item():.3e}, max d/bound {(d / bound).max().item():.3f}")
    assert bool((d <= bound).all()), f"{case}: max excess {(d - bound).max().item():.3e}"
    inside = r["full_x0"].abs() < 1.0
    assert bool(inside.any()) and not bool(inside.all())
    assert torch.equal(r["full"][inside], r["full_clipped"][inside]), f"{case}: the clip acted inside (-1, 1)"
    assert not torch.equal(r["full"], r["full_clipped"])
    # 3. sg == 0: z is neither drawn nor read
    assert torch.isfinite(r["det_nan"]).all()
    assert torch.equal(r["det_nan"], r["det_zero"])
    assert torch.equal(r["row0_nan"], r["row0_zero"]) and torch.isfinite(r["row0_nan"]).all()
    # 4. Philox keyed (seed, row, noise_offset + element)
    assert r["sg2"] > 0.0
    for got, inj in zip(r["philox"], r["injected"]):
        assert torch.equal(got, inj), f"{case}: max|d| {(got - inj).abs().max().item():.3e}"
    assert not torch.equal(r["philox"][0], r["philox"][1])


# ----------------------------------------------------------------------------- 5. row -> timestep
@pytest.mark.parametrize("arch", ["ddpm", "cfg"])
def test_predict_x0_row_is_its_timestep(arch):
    a = TINY_CFG if arch == "cfg" else ARCH_TINY
    base = _sampler(a)
    s = _ddim(base, eta=0.5, clip_x0=True)
    x, lab = _x(2, seed=5), _labels(a, 2)
    for k, t in enumerate(TAU):
        got = s.predict_x0(x, k, labels=lab)
        want = base.predict_x0(x, t, labels=lab)
        assert torch.equal(got, want), f"{arch} row {k} (t = {t}): max|d| {(got - want).abs().max().item():.3e}"
    assert not torch.equal(base.predict_x0(x, 2, labels=lab), base.predict_x0(x, 3, labels=lab))
    with pytest.raises(ValueError):
        s.predict_x0(x, K, labels=lab)


# ----------------------------------------------------------------------------- 6. the loop
def test_loop_graph_eager_single_rows_and_form_switch():
    base = _sampler(ARCH_TINY)  # its own handle
    s = _ddim(base, eta=0.5, clip_x0=True)
    x = _x(3, seed=7)
    before_ddpm = base.run(x.clone(), seed=SEED)
    nat = s._native(3)
    caps = nat.query("graph_captures")
    g = s.run(x.clone(), seed=SEED, graph=True)
    assert nat is s._native(3) and nat.query("graph_captures") == caps + 1
    e = s.run(x.clone(), seed=SEED, graph=False)
    one = x.clone()
    for k in range(K - 1, -1, -1):
        s.run(one, t_begin=k, t_end=k, seed=SEED, clip=(k == 0))
    assert nat.query("graph_captures") == caps + 1, "the single-row runs replay the loop's graph"
    assert torch.equal(g, e) and torch.equal(g, one)
    assert torch.isfinite(g).all() and float(g.abs().max()) <= 1.0 and not torch.equal(g, x)
    # both samplers alive on one handle: each re-installs its own schedule; no stale graph, no stale tables
    after_ddpm = base.run(x.clone(), seed=SEED)
    assert base._native(3) is nat and nat.query("sched_form") == 0 and nat.query("T_sched") == T
    assert torch.equal(before_ddpm, after_ddpm) and not torch.equal(after_ddpm, g)
    assert torch.equal(s.run(x.clone(), seed=SEED), g) and nat.query("sched_form") == 1
    # the NaN flag
    Z = torch.randn((K,) + tuple(x.shape), generator=torch.Generator().manual_seed(1)).to(DEV)
    want = s.run(x.clone(), t_begin=2, t_end=2, noise=Z, clip=False)
    bad = Z.clone()
    bad[2, 2, 1, 5, 7] = float("nan")
    for graph in (True, False):
        with pytest.raises(AssertionError, match="nan in tensor"):
            s.run(x.clone(), t_begin=2, t_end=2, noise=bad, clip=False, graph=graph)
    assert torch.equal(s.run(x.clone(), t_begin=2, t_end=2, noise=Z, clip=False), want)
    other = Z.clone()
    other[3, 2, 1, 5, 7] = float("nan")  # a draw of a row that is not run
    assert torch.equal(s.run(x.clone(), t_begin=2, t_end=2, noise=other, clip=False), want)


# ----------------------------------------------------------------------------- 7. the whole loop against the oracle
def _oracle_loop(a, sd, x, Z, rows, labels, w):
    """The x0-form loop in fp64 around oracle.ref_cpu's UNet forward: K rows, eta and clip_x0 as the rows say."""
    sd = {k: v.double() for k, v in sd.items()}

    def net(xx, tt, ll=None):
        return R.unet_forward(sd, xx, tt, a.ch, a.ch_mult, a.attn, a.num_res_blocks, labels=ll, cfg=a.cfg)

    x = x.double()
    with torch.no_grad():
        for k in range(K - 1, -1, -1):
            t = torch.full((x.shape[0],), TAU[k], dtype=torch.long)
            if a.cfg:
                e = (1.0 + w) * net(x, t, labels) - w * net(x, t, torch.zeros_like(labels))
            else:
                e = net(x, t)
            x0 = (rows["a0"][k] * x - rows["b0"][k] * e).clamp(-1, 1)
            x = rows["c0"][k] * x0 + rows["cx"][k] * x + rows["sg"][k] * Z[k].double()
    return x.clamp(-1, 1)


@pytest.fixture(scope="module")
def oracle_runs():
    out = {}
    for arch, a in (("ddpm", ARCH_TINY), ("cfg", TINY_CFG)):
        g = torch.Generator().manual_seed(11)
        x = torch.randn(2, 3, 32, 32, generator=g)
        Z = torch.randn(K, 2, 3, 32, 32, generator=g)
        lab = torch.tensor([3, 7]) if a.cfg else None
        base = _sampler(a)
        rows = _ddim(base, eta=0.5, clip_x0=True).rows
        out[arch] = (x, Z, lab, _oracle_loop(a, synthetic_state_dict(a, 0), x, Z, rows, lab, base.w))
    return out


@pytest.mark.parametrize("arch", ["ddpm", "cfg"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_whole_loop_vs_oracle(oracle_runs, arch, precision):
    a = TINY_CFG if arch == "cfg" else ARCH_TINY
    x, Z, lab, want = oracle_runs[arch]
    s = _ddim(_sampler(a, precision), eta=0.5, clip_x0=True)
    got = s.run(x.to(DEV).clone(), labels=None if lab is None else lab.to(DEV), noise=Z.to(DEV)).cpu().double()
    d = got - want
    mx, l2 = float(d.abs().max()), float(d.norm() / want.norm())
    print(f"{arch} {precision}: max|d| {mx:.3e}, relative L2 {l2:.3e}")
    if precision == "fp32":
        assert mx <= 2e-3
    else:
        assert l2 <= 3e-2


# ----------------------------------------------------------------------------- 8. the searches, in rows
@pytest.fixture(scope="module")
def ddim_fp32():
    return _ddim(_sampler(ARCH_TINY), eta=0.5, clip_x0=True)


def _round_by_hand(eng, smp, round_id, n, pivot=None, scale=1.0):
    x = eng.candidate_noise(round_id, 0, n, SHAPE, pivot, scale)
    smp.run(x, seed=(eng.seed * 1000003 + round_id) & MASK62, noise_offset=0)
    return x


def test_random_and_zero_order_search_on_rows(ddim_fp32):
    ver, n = OracleVerifier(), 4
    eng = SearchEngine(ddim_fp32, ver, seed=4)
    _, score, h = eng.random_search(n, SHAPE)
    x = _round_by_hand(eng, ddim_fp32, 0, n)
    own = [float(ver.score_batch(x[i:i + 1], 1)[0]) for i in range(n)]
    assert max(abs(p - q) for p, q in zip(h["scores"], own)) <= 1e-6
    assert h["scores"] == ver.score_batch(x, n).cpu().tolist() and score == max(h["scores"])
    assert torch.equal(eng.best_image, x[h["best_index"]:h["best_index"] + 1])
    init = eng.initial_noise(SHAPE)
    _, score, h = eng.zero_order_search(init, n, 0.95, 1)
    x = _round_by_hand(eng, ddim_fp32, 1, n, pivot=init, scale=1 - 0.95)
    own = [float(ver.score_batch(x[i:i + 1], 1)[0]) for i in range(n)]
    assert max(abs(p - q) for p, q in zip(h["scores"][0], own)) <= 1e-6
    assert h["scores"][0] == ver.score_batch(x, n).cpu().tolist()
    assert torch.equal(eng.best_image, x[h["best_index"][0]:h["best_index"][0] + 1])


def test_noop_stage_at_row_2_is_the_placeholder_round(ddim_fp32, monkeypatch):
    ver, n = OracleVerifier(), 4
    eng = SearchEngine(ddim_fp32, ver, seed=4)
    init = eng.initial_noise(SHAPE)
    rb, rs, rh = eng.path_search(init, n, 0.1, 2)
    rimg = eng.best_image.clone()
    real, calls = ver.score_batch, []

    def fake(images, n_cand):
        calls.append(n_cand)
        if len(calls) == 1:  # the stage's scores: descending, so parents = identity
            return torch.arange(n_cand, 0, -1, dtype=torch.float64, device=images.device)
        return real(images, n_cand)

    monkeypatch.setattr(ver, "score_batch", fake)
    b, s, h = eng.path_search_branch(init, n, 0.1, [2], keep=n, renoise_steps=0)
    assert h["parents"] == [[0, 1, 2, 3]] and len(calls) == 2
    assert h["scores"] == rh["scores"] and h["best_index"] == rh["best_index"] and s == rs
    assert torch.equal(b, rb) and torch.equal(eng.best_image, rimg)
    assert h["unet_steps"] == n * (K + 1)


def test_branching_search_on_rows(ddim_fp32):
    n, res = 4, []
    for _ in range(2):
        eng = SearchEngine(ddim_fp32, OracleVerifier(), seed=6)
        init = eng.initial_noise(SHAPE)
        _, s, h = eng.path_search_branch(init, n, 0.5, [2], keep=n // 2, renoise_steps=1)
        res.append((s, h, eng.best_image.clone()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and torch.equal(res[0][2], res[1][2])
    h = res[0][1]
    # rows 3 (window 0: 3 .. s + 1), then rows s + 1 .. 0 again after the branch (4), plus one x0 evaluation
    assert h["unet_steps"] == n * ((1 + 4) + 1)
    assert len(set(h["parents"][0])) == n // 2 and torch.isfinite(torch.tensor(h["scores"])).all()
    for kw in (dict(injection_steps=[K]), dict(injection_steps=[3], renoise_steps=1), dict(injection_steps=[0])):
        with pytest.raises(ValueError):  # rows: s + renoise_steps <= K - 1, s >= 1
            eng.path_search_branch(init, n, 0.5, **{"keep": 2, "renoise_steps": 0, **kw})


def test_reference_noise_is_refused(ddim_fp32):
    with pytest.raises(ValueError, match="reference"):
        SearchEngine(ddim_fp32, OracleVerifier(), seed=1, noise="reference")
    with pytest.raises(ValueError, match="reference"):
        ddim_fp32.denoise_fn(reference_rng=True)
