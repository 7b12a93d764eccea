"""GPU tests of the second-order few-step sampler: the 2M step epilogue of every tail kernel (TailArgs::step_mode 6 and,
traced, 7), the schedule and the x0 history behind it (itsd_set_schedule_x0_2m, ITSD_RUN_CONTINUE), and the searches on
it. T = 12 and K = 4 rows (tau = 2, 5, 8, 11); the six tail forms are TAIL_CASES of test_gpu_path_branch.py, whose
docstring names the kernel each one runs.

The step is, in fp32 with contraction off,
    x0 = a0 x - b0 e  (clipped iff clip_x0)
    cp != 0:  x0p = restart ? x0 : hist;   m = ((c0 x0) + (cp x0p)) + (cx x)
    cp == 0:  m = (c0 x0) + (cx x)
    hist = x0;   x' = sg != 0 ? m + sg z : m
so torch repeats it exactly from predict_x0 (the same a0 x - b0 e, clipped: every sampler here has clip_x0=True) and
the fp32 casts of the row, and everything that compares two runs of one program is bit equality.

The two checks that are not: the trace rows against predict_x0's moments use test_gpu_x0_trace.py's own derived bound
(_check_row with L_CHAIN), and the whole loop against the fp64 oracle uses DESIGN section 4's bounds for trajectories of
T <= 20 steps, the ones test_whole_loop_vs_oracle uses: fp32 max-abs <= 2e-3, bf16 relative L2 <= 3e-2."""
import itertools

import pytest
import torch

from itsd import runtime as rt
from itsd.arch import ARCH_TINY
from itsd.schedule import adam_coeffs, x0_coeffs, x0_form_rows
from itsd.search import SearchEngine, es_weights, strict_argmax
from itsd.verifier import OracleVerifier
from itsd.weights import synthetic_state_dict
from oracle import ref_cpu as R
from test_gpu_path_branch import DEV, MASK62, TAIL_CASES, TINY_CFG, T, _sampler, _x
from test_gpu_sampler_x0 import K, SEED, SHAPE, TAU, _ddim, _labels, _row
from test_gpu_x0_trace import L_CHAIN, _check_row

pytestmark = pytest.mark.gpu


def _2m(smp, steps=K, clip_x0=True):
    """A second-order few-step sampler over the net (and the schedule) of the ancestral sampler smp."""
    return type(smp)(smp.model, smp.sched.beta_1, smp.sched.beta_T, T, w=smp.w, sampler="dpmpp2m", steps=steps,
                     clip_x0=clip_x0)


def _step2(row, x0, x0p, x):
    """Row's 2M expression in torch fp32: separate multiplies and adds, the kernel's association."""
    return ((row["c0"] * x0) + (row["cp"] * x0p)) + row["cx"] * x


def _invalid(fn):
    with pytest.raises(rt.ItsdError) as e:
        fn()
    assert e.value.code == rt.ITSD_ERR_INVALID, str(e.value)
    return str(e.value)


# ----------------------------------------------------------------------------- 5, 6, 11: every tail form
_FORMS = {}


def _forms(case):
    """Every run the per-form checks compare, made once inside the form's io_mfma window on one handle."""
    if case in _FORMS:
        return _FORMS[case]
    a, precision, io_mfma, n = TAIL_CASES[case]
    rt.set_option("io_mfma", io_mfma)
    try:
        s = _2m(_sampler(a, precision))
        x, lab = _x(n, a.img_size, seed=3), _labels(a, n)
        nat = s._native(n)
        r = {"x": x, "n": n}
        # 6. the whole run on the fresh handle (its history is whatever the allocation held)
        r["whole_fresh"] = s.run(x.clone(), labels=lab)
        r["form"] = (nat.query("sched_form"), nat.query("T_sched"))
        # 5. row 3, then row 2 continued
        r["x0_3"] = s.predict_x0(x, 3, labels=lab)
        r["x3"] = s.run(x.clone(), t_begin=3, t_end=3, labels=lab, clip=False)
        r["x0_2"] = s.predict_x0(r["x3"], 2, labels=lab)  # (between the two runs: it leaves the history alone)
        r["x2"] = s.run(r["x3"].clone(), t_begin=2, t_end=2, labels=lab, clip=False, cont=True)
        r["rows"] = [_row(s, k) for k in range(K)]
        # 6. restart: row 2 alone after a poison, then the whole run after another
        nat.poison(x.device)
        r["x2_restart"] = s.run(r["x3"].clone(), t_begin=2, t_end=2, labels=lab, clip=False)
        nat.poison(x.device)
        r["whole_poisoned"] = s.run(x.clone(), labels=lab)
        # 11. the trace: a traced whole run, and row by row with the x0 of each row's input
        r["trace"] = s.new_trace(n)
        r["whole_traced"] = s.run(x.clone(), labels=lab, trace=r["trace"])
        xs, by_row, x0s = x.clone(), s.new_trace(n), []
        for k in range(K - 1, -1, -1):
            x0s.append(s.predict_x0(xs, k, labels=lab))
            s.run(xs, t_begin=k, t_end=k, labels=lab, clip=(k == 0), trace=by_row, cont=(k != K - 1))
        r["x0_rows"], r["by_row"], r["by_row_x"] = x0s[::-1], by_row, xs
        # 5. once more through the raw binding: eta = 0.5's sg on the same c0 / cp / cx, injected noise
        rows = {**s.rows, "sg": x0_form_rows(s.sched.alphas_bar, TAU, 0.5)["sg"]}
        nat.set_schedule_x0_2m(TAU, rows, True, s.w)
        nat._sched_args = None  # (a sampler that runs on this handle later installs its own again)
        Z = torch.randn((K,) + tuple(x.shape), generator=torch.Generator().manual_seed(17)).to(DEV)
        r["Z"], r["sg"] = Z, [rows["sg"][k].float().to(DEV) for k in range(K)]
        r["n3"] = x.clone()
        nat.run(r["n3"], 3, 3, 0, noise=Z, labels=lab, clip=False)
        a0, b0 = x0_coeffs(s.sched.alphas_bar, TAU[2])
        r["n_x0_2"] = nat.predict_x0(r["n3"], 2, a0, b0, torch.empty_like(x), labels=lab)
        r["n2"] = r["n3"].clone()
        nat.run(r["n2"], 2, 2, 0, noise=Z, labels=lab, clip=False, cont=True)
    finally:
        rt.set_option("io_mfma", 1)
    _FORMS[case] = r
    return r


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_2m_step_every_tail_form(case):
    r = _forms(case)
    x, rows = r["x"], r["rows"]
    assert r["form"] == (2, K)
    assert float(rows[2]["cp"]) != 0.0 and float(rows[1]["cp"]) != 0.0
    assert float(rows[3]["cp"]) == 0.0 and float(rows[0]["cp"]) == 0.0
    for name in ("x0_3", "x0_2"):
        rail = float((r[name].abs() == 1.0).float().mean())
        print(f"{case}: share of {name} on a rail {rail:.3f}")
        assert 0.01 <= rail <= 0.99, f"{case}: {rail:.3f} of {name} on a rail: one branch of the clip is not seen"
    # row 3 is first order (cp == 0), row 2 continued is second order on row 3's x0
    want3 = (rows[3]["c0"] * r["x0_3"]) + (rows[3]["cx"] * x)
    assert torch.equal(r["x3"], want3), f"{case}: row 3 max|d| {(r['x3'] - want3).abs().max().item():.3e}"
    want2 = _step2(rows[2], r["x0_2"], r["x0_3"], r["x3"])
    assert torch.equal(r["x2"], want2), f"{case}: row 2 max|d| {(r['x2'] - want2).abs().max().item():.3e}"
    assert not torch.equal(r["x0_2"], r["x0_3"])
    # the raw binding, with noise: + sg z on both rows
    assert all(float(v) > 0.0 for v in r["sg"][1:])
    Z, n3 = r["Z"], r["n3"]
    want = ((rows[3]["c0"] * r["x0_3"]) + (rows[3]["cx"] * x)) + r["sg"][3] * Z[3]
    assert torch.equal(n3, want), f"{case}: noisy row 3 max|d| {(n3 - want).abs().max().item():.3e}"
    want = _step2(rows[2], r["n_x0_2"], r["x0_3"], n3) + r["sg"][2] * Z[2]
    assert torch.equal(r["n2"], want), f"{case}: noisy row 2 max|d| {(r['n2'] - want).abs().max().item():.3e}"


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_restart_never_reads_the_history(case):
    r = _forms(case)
    row = r["rows"][2]
    assert bool(torch.isfinite(r["x2_restart"]).all())
    want = _step2(row, r["x0_2"], r["x0_2"], r["x3"])
    assert torch.equal(r["x2_restart"], want), f"{case}: max|d| {(r['x2_restart'] - want).abs().max().item():.3e}"
    assert not torch.equal(r["x2_restart"], r["x2"])
    # rows K - 1 and 0 never read it either: the poisoned handle's whole run is the fresh handle's
    assert bool(torch.isfinite(r["whole_fresh"]).all()) and float(r["whole_fresh"].abs().max()) <= 1.0
    assert torch.equal(r["whole_poisoned"], r["whole_fresh"])


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_trace_rows_are_each_rows_own_x0(case):
    r = _forms(case)
    assert torch.equal(r["whole_traced"], r["whole_fresh"]), f"{case}: the traced run moved x"
    assert torch.equal(r["by_row_x"], r["whole_fresh"]) and torch.equal(r["by_row"], r["trace"]), f"{case}: row by row"
    for k in range(K):
        _check_row(f"{case} row {k}", r["trace"][k], r["x0_rows"][k], L_CHAIN[case])
    assert torch.equal(r["whole_fresh"], r["x0_rows"][0]), f"{case}: the output is not row 0's x0"


# ----------------------------------------------------------------------------- 7. split equals whole
@pytest.fixture(scope="module")
def two_m():
    return _2m(_sampler(ARCH_TINY))


def test_split_with_cont_equals_whole(two_m):
    s, x = two_m, _x(3, seed=7)
    nat = s._native(3)
    whole = s.run(x.clone(), graph=True)
    assert torch.equal(s.run(x.clone(), graph=False), whole)
    for g1, g2 in itertools.product((True, False), repeat=2):
        y = s.run(x.clone(), t_begin=3, t_end=2, clip=False, graph=g1)
        caps = nat.query("graph_captures")
        s.run(y, t_begin=1, t_end=0, cont=True, graph=g2)
        assert nat.query("graph_captures") == caps, "the continued run captured a graph of its own"
        assert torch.equal(y, whole), f"graph {g1}, {g2}: max|d| {(y - whole).abs().max().item():.3e}"
    y = s.run(x.clone(), t_begin=3, t_end=2, clip=False)
    s.run(y, t_begin=1, t_end=0)  # restarted: row 1 uses its own x0 twice
    assert bool(torch.isfinite(y).all()) and not torch.equal(y, whole)


# ----------------------------------------------------------------------------- 8. K = 2 is ddim
def test_two_rows_are_ddim_and_the_forms_replace_one_another():
    base = _sampler(ARCH_TINY)  # its own handle
    m, d = _2m(base, steps=2), _ddim(base, steps=2, eta=0.0, clip_x0=True)
    assert bool((m.rows["cp"] == 0).all())
    x = _x(3, seed=9)
    nat = m._native(3)
    first = m.run(x.clone())
    assert nat.query("sched_form") == 2 and nat.query("T_sched") == 2
    ddim = d.run(x.clone())
    assert d._native(3) is nat and nat.query("sched_form") == 1
    again = m.run(x.clone())
    assert nat.query("sched_form") == 2
    assert torch.equal(first, ddim) and torch.equal(again, first)
    assert torch.equal(d.run(x.clone()), ddim) and nat.query("sched_form") == 1
    anc = base.run(x.clone(), seed=SEED)
    assert nat.query("sched_form") == 0 and not torch.equal(anc, first)


# ----------------------------------------------------------------------------- 9. refusals at run time
def test_cont_refusals(two_m):
    base = _sampler(ARCH_TINY)
    x = _x(3, seed=11)
    keep = x.clone()
    for smp in (base, _ddim(base, eta=0.0, clip_x0=True)):  # the other two forms
        smp.run(x.clone(), t_begin=3, t_end=3, seed=SEED, clip=False)
        assert "ITSD_RUN_CONTINUE" in _invalid(lambda: smp.run(x, t_begin=2, t_end=2, seed=SEED, cont=True))
    s = _2m(base)
    nat = s._native(3)
    # right after a schedule install: the history holds nothing
    nat._sched_args = None
    s._native(3)
    assert nat.query("sched_form") == 2
    assert "none" in _invalid(lambda: s.run(x, t_begin=2, t_end=2, cont=True))
    caps = nat.query("graph_captures")
    s.run(x.clone(), t_begin=3, t_end=2, clip=False)
    assert "top row" in _invalid(lambda: s.run(x, t_begin=3, t_end=3, cont=True))
    assert "row 2" in _invalid(lambda: s.run(x, t_begin=2, t_end=2, cont=True))    # the run ended on row 2, not 3
    assert "row 2" in _invalid(lambda: s.run(x, t_begin=0, t_end=0, cont=True))
    assert "3 images" in _invalid(lambda: s.run(x[:2], t_begin=1, t_end=1, cont=True))  # another n
    assert nat.query("graph_captures") == caps + 1 and torch.equal(x, keep), "a refused run launched something"
    s.run(x.clone(), t_begin=1, t_end=1, cont=True, clip=False)  # the one continuation that is valid


# ----------------------------------------------------------------------------- 10. batch independence
def test_image_alone_equals_image_in_a_batch(two_m):
    s = two_m
    x = _x(3, seed=13)
    batch = s.run(x.clone())
    alone = s.run(x[2:3].clone())
    assert torch.equal(alone, batch[2:3]), f"max|d| {(alone - batch[2:3]).abs().max().item():.3e}"
    moved = s.run(torch.cat([x[1:2], x[0:1], x[2:3]]).contiguous())
    assert torch.equal(moved[0], batch[1]) and torch.equal(moved[1], batch[0])


# ----------------------------------------------------------------------------- 12. the whole loop against the oracle
def _oracle_loop(a, sd, x, rows, labels, w):
    """The 2M recursion in fp64 around oracle.ref_cpu's UNet forward: K rows, clip_x0, a restart at the top row."""
    sd = {k: v.double() for k, v in sd.items()}

    def net(xx, tt, ll=None):
        return R.unet_forward(sd, xx, tt, a.ch, a.ch_mult, a.attn, a.num_res_blocks, labels=ll, cfg=a.cfg)

    x, prev = x.double(), None
    with torch.no_grad():
        for k in range(K - 1, -1, -1):
            t = torch.full((x.shape[0],), TAU[k], dtype=torch.long)
            if a.cfg:
                e = (1.0 + w) * net(x, t, labels) - w * net(x, t, torch.zeros_like(labels))
            else:
                e = net(x, t)
            x0 = (rows["a0"][k] * x - rows["b0"][k] * e).clamp(-1, 1)
            x = rows["c0"][k] * x0 + rows["cp"][k] * (x0 if prev is None else prev) + rows["cx"][k] * x
            prev = x0
    return x.clamp(-1, 1)


@pytest.fixture(scope="module")
def oracle_runs():
    out = {}
    for arch, a in (("ddpm", ARCH_TINY), ("cfg", TINY_CFG)):
        x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(11))
        lab = torch.tensor([3, 7]) if a.cfg else None
        base = _sampler(a)
        out[arch] = (x, lab, _oracle_loop(a, synthetic_state_dict(a, 0), x, _2m(base).rows, lab, base.w))
    return out


@pytest.mark.parametrize("arch", ["ddpm", "cfg"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_whole_loop_vs_oracle(oracle_runs, arch, precision):
    a = TINY_CFG if arch == "cfg" else ARCH_TINY
    x, lab, want = oracle_runs[arch]
    s = _2m(_sampler(a, precision))
    got = s.run(x.to(DEV).clone(), labels=None if lab is None else lab.to(DEV)).cpu().double()
    d = got - want
    mx, l2 = float(d.abs().max()), float(d.norm() / want.norm())
    print(f"{arch} {precision}: max|d| {mx:.3e}, relative L2 {l2:.3e}")
    if precision == "fp32":
        assert mx <= 2e-3
    else:
        assert l2 <= 3e-2


# ----------------------------------------------------------------------------- 13. the searches
def test_random_search_round_by_hand(two_m):
    ver, n = OracleVerifier(), 4
    eng = SearchEngine(two_m, ver, seed=4)
    _, score, h = eng.random_search(n, SHAPE)
    x = eng.candidate_noise(0, 0, n, SHAPE, None, 1.0)
    two_m.run(x, seed=(eng.seed * 1000003 + 0) & MASK62, noise_offset=0)
    assert h["scores"] == ver.score_batch(x, n).cpu().tolist() and score == max(h["scores"])
    assert torch.equal(eng.best_image, x[h["best_index"]:h["best_index"] + 1])
    init = eng.initial_noise(SHAPE)
    _, score, h = eng.zero_order_search(init, n, 0.95, 1)
    x = eng.candidate_noise(1, 0, n, SHAPE, init, 1 - 0.95)
    two_m.run(x, seed=(eng.seed * 1000003 + 1) & MASK62, noise_offset=0)
    assert h["scores"][0] == ver.score_batch(x, n).cpu().tolist()
    # the placeholder path search is one such round too
    _, ps, ph = eng.path_search(init, n, 0.1, 2)
    assert ps == max(ph["scores"]) and torch.isfinite(torch.tensor(ph["scores"])).all()


def test_gradient_search_by_hand(two_m):
    smp, sigma = two_m, 0.05
    seed, n_pairs, iters, lr = 4, 2, 2, 0.01
    n, per = 2 * n_pairs, 3 * 32 * 32
    ver = OracleVerifier()
    eng = SearchEngine(smp, ver, seed=seed)
    init = eng.initial_noise(SHAPE)
    best, score, h = eng.gradient_search(init, n_pairs, sigma, iters, lr=lr)
    image = eng.best_image.clone()
    theta = init.clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    ws = torch.empty(rt.es_workspace_bytes(n_pairs, per), dtype=torch.uint8, device=DEV)
    b_noise, b_score, b_image, scores = None, float("-inf"), None, []
    for it in range(iters):
        sid = 0xB0000000 + 1 + it
        xT = rt.es_candidates(torch.empty(n, 3, 32, 32, device=DEV), theta, n, sigma, seed, sid)
        x = xT.clone()
        smp.run(x, seed=(seed * 1000003 + 1 + it) & MASK62, noise_offset=0)
        sc = ver.score_batch(x, n).cpu()
        bi, bs = strict_argmax(sc)
        scores.append(sc.tolist())
        if bs > b_score:
            b_score, b_noise, b_image = bs, xT[bi:bi + 1].clone(), x[bi:bi + 1].clone()
        rt.es_step(theta, m, v, es_weights(sc, sigma).to(DEV), seed, sid, adam_coeffs(lr, (0.9, 0.999), 1e-8, it + 1), ws)
    assert h["scores"] == scores and score == b_score
    assert torch.equal(best, b_noise) and torch.equal(image, b_image)
    assert len(set(scores[0])) == n


def test_branching_search_windows_are_restarted_runs(two_m, monkeypatch):
    n, calls = 4, []
    real = two_m.run

    def spy(x, *args, **kw):
        calls.append((kw.get("t_begin"), kw.get("t_end"), bool(kw.get("cont", False))))
        return real(x, *args, **kw)

    monkeypatch.setattr(two_m, "run", spy)
    res = []
    for _ in range(2):
        eng = SearchEngine(two_m, OracleVerifier(), seed=6)
        init = eng.initial_noise(SHAPE)
        _, s, h = eng.path_search_branch(init, n, 0.5, [2], keep=n // 2, renoise_steps=1)
        res.append((s, h, eng.best_image.clone()))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and torch.equal(res[0][2], res[1][2])
    h = res[0][1]
    assert h["unet_steps"] == n * ((1 + 4) + 1) and torch.isfinite(torch.tensor(h["scores"])).all()
    assert calls[:2] == [(3, 3, False), (3, 0, False)], calls  # the window before the branch, the one after it


def test_particle_search_refuses_the_deterministic_sampler(two_m):
    eng = SearchEngine(two_m, OracleVerifier(), seed=1)
    with pytest.raises(ValueError, match="dpmpp2m"):
        eng.fk_search(eng.initial_noise(SHAPE), 4, 0.5, [2], 1.0)
    with pytest.raises(ValueError, match="reference"):
        SearchEngine(two_m, OracleVerifier(), seed=1, noise="reference")
