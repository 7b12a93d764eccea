"""GPU tests of the guidance schedules (itsd_set_guidance): the table-guided x0-form step of every tail kernel, the
cond-only step program of w = 0 rows, refusals and lifetime, and one search over per-candidate scales. The tiny CFG arch
with T = 12 and K = 4 rows (tau = 2, 5, 8, 11) on the three CFG forms of test_gpu_path_branch.py's TAIL_CASES: 32 px for
tail2_kernel (fp32) and tail_mfma_kernel (bf16), 128 px for the generic tail_kernel; batches of 2 and 3.

Under a table the step guides with, in fp32 and without contraction,
    w = w_rows[k] (* m[img]);  w1 = 1.0f + w;  e = w1 ec - w eu
and then runs the mode's own step. 1.0f + w and the scalar path's (float)(1.0 + (double)w) round alike (the double sum
of two fp32 values is exact), so whatever compares a table run with a scalar run of the same program is bit equality.

Two checks are not bit equality:

* a cond-only row against the forward API (check 4). The cond-only step is
      x0 = clip(a0 x - b0 e);  m = (c0 x0) + (cx x);  x' = m + sg z
  on the forward's own e (the same program at batch n). With one ulp, EPS = 2^-23 relative, for each of its
  operations, as test_gpu_path_branch.py's header counts them: x0 errs by at most EPS (|a0 x| + |b0 e|) (two products
  and a difference, half an ulp each, |x0| <= |a0 x| + |b0 e|; the clip does not expand it), which c0 scales; each of
  the three products c0 x0, cx x, sg z and the two sums adds EPS of its own result, and |m| <= |c0 x0| + |cx x|:
      |d| <= EPS (|c0| (|a0 x| + |b0 e|) + 3 |c0 x0| + 3 |cx x| + 2 |sg z|)
  with every magnitude taken in fp64 from the fp32 operands. A derived bound, not a measured one.
* the cond-only program against the doubled batch through the table (w = 0 on both sides), and the whole loop against
  the fp64 oracle (check 5): the project's tolerances for K = 4 x0-form loops (test_whole_loop_vs_oracle, DESIGN
  section 4): fp32 max-abs <= 2e-3, bf16 relative L2 <= 3e-2. The two programs pick kernels by batch, so bit equality
  is not promised. The oracle loop runs at 32 px (both precisions); the 128 px form is held to the scalar path's bits
  by checks 1-4 (an fp64 UNet at 128 px costs half a minute on the CPU)."""
import json

import pytest
import torch

from itsd import entry as E
from itsd import runtime as rt
from itsd.arch import ARCH_TINY
from itsd.diffusion import CondGaussianDiffusionSampler
from itsd.model import CondUNet
from itsd.schedule import guidance_rows
from itsd.search import SearchEngine
from itsd.verifier import OracleVerifier
from itsd.weights import synthetic_state_dict
from oracle import ref_cpu as R
from test_gpu_path_branch import DEV, MASK62, TAIL_CASES, TINY_CFG, T, _sampler, _x

pytestmark = pytest.mark.gpu

K = 4
TAU = [2, 5, 8, 11]
SEED = 0x5EED
EPS = 2.0 ** -23
W = 1.8
CFG_CASES = ["tail_f32_cfg_128px", "tail2_f32_cfg", "tail_mfma_cfg"]


def _mk(base, kind="ddim", w=None, guidance=None):
    """A few-step conditional sampler over the net of base: ddim (eta 0.5, clip_x0) or dpmpp2m (clip_x0)."""
    kw = dict(sampler=kind, steps=K, clip_x0=True)
    if kind == "ddim":
        kw["eta"] = 0.5
    return CondGaussianDiffusionSampler(base.model, base.sched.beta_1, base.sched.beta_T, T,
                                        w=base.w if w is None else w, guidance=guidance, **kw)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _labels(n):
    return torch.tensor([3, 7, 5], dtype=torch.int32, device=DEV)[:n]


def _noise(x, seed=17):
    return torch.randn((K,) + tuple(x.shape), generator=torch.Generator().manual_seed(seed)).to(DEV)


class _Case:
    """One tail form: the base (ancestral, w = 1.8) sampler over a fresh net, made inside the form's io_mfma window."""

    def __init__(self, case):
        self.a, self.precision, self.io_mfma, self.n = TAIL_CASES[case]
        self.case = case

    def __enter__(self):
        rt.set_option("io_mfma", self.io_mfma)
        self.base = _sampler(self.a, self.precision)
        assert self.base.w == W
        return self

    def __exit__(self, *exc):
        rt.set_option("io_mfma", 1)
        rt.set_option("cfg_skip", 1)
        return False


# ----------------------------------------------------------------------------- 1. a constant table is the scalar path
@pytest.mark.parametrize("case", CFG_CASES)
def test_constant_table_is_the_scalar_path(case):
    with _Case(case) as c:
        x, lab = _x(c.n, c.a.img_size, seed=3), _labels(c.n)
        for kind in ("ddim", "dpmpp2m"):
            scalar = _mk(c.base, kind)
            table = _mk(c.base, kind, guidance=guidance_rows(TAU, W, "constant"))
            # the four step modes (ddim, ddim traced, 2M, 2M traced), each replayed from its graph or run eagerly
            forms = [(False, True), (True, False)] if kind == "ddim" else [(False, False), (True, True)]
            out = {}
            for s in (scalar, table):  # (each sampler's runs together: one schedule install a sampler)
                for traced, graph in forms:
                    tr = s.new_trace(c.n) if traced else None
                    out[s is table, traced, graph] = (s.run(x.clone(), labels=lab, seed=SEED, graph=graph, trace=tr), tr)
                    assert s._native(c.n).query("guidance") == (1 if s is table else 0)
                    assert s._native(c.n).query("cond_only_steps") == 0
            for traced, graph in forms:
                (got, gtr), (want, wtr) = out[True, traced, graph], out[False, traced, graph]
                tag = f"{case} {kind} traced={traced} graph={graph}"
                assert torch.equal(got, want), f"{tag}: max|d| {(got - want).abs().max().item():.3e}"
                if traced:
                    assert torch.isfinite(wtr).all() and torch.equal(gtr, wtr), f"{tag}: the trace"
            assert table.last_unet_evals_per_image == 2 * K == table.unet_evals_per_image()
            assert not torch.equal(out[(True,) + forms[0]][0], x)


# ----------------------------------------------------------------------------- 2. per row
@pytest.mark.parametrize("case", CFG_CASES)
def test_per_row_weights(case):
    rows = [0.9, 1.8, 0.45, 1.8]
    with _Case(case) as c:
        x, lab = _x(c.n, c.a.img_size, seed=4), _labels(c.n)
        Z = _noise(x)
        table = _mk(c.base, guidance=rows)
        outs = [table.run(x.clone(), t_begin=k, t_end=k, labels=lab, noise=Z, clip=False) for k in range(K)]
        for k in range(K):
            want = _mk(c.base, w=rows[k]).run(x.clone(), t_begin=k, t_end=k, labels=lab, noise=Z, clip=False)
            assert torch.equal(outs[k], want), f"{case} row {k}: max|d| {(outs[k] - want).abs().max().item():.3e}"
        # rows 1 and 3 share the weight but not the timestep; rows 0 and 2 differ in both
        assert not torch.equal(outs[1], outs[3]) and not torch.equal(outs[0], outs[2])


# ----------------------------------------------------------------------------- 3. per image
@pytest.mark.parametrize("case", CFG_CASES)
def test_per_image_multipliers(case):
    n, m = 3, [1.0, 0.5, 0.25]
    with _Case(case) as c:
        one = _x(1, c.a.img_size, seed=5)
        x = one.repeat(n, 1, 1, 1).contiguous()  # the same image three times, under one label and one noise field
        lab = torch.full((n,), 3, dtype=torch.int32, device=DEV)
        Z = _noise(one, seed=19).repeat(1, n, 1, 1, 1).contiguous()
        for kind in ("ddim", "dpmpp2m"):
            table = _mk(c.base, kind, guidance=guidance_rows(TAU, W, "constant"))
            got = table.run(x.clone(), labels=lab, noise=Z, guidance_scale=_f32(m))
            assert table.model.native(n).query("guidance") == 2  # (the handle itself: _native would re-install)
            for i in range(n):
                wi = (_f32(W) * _f32(m[i])).item()  # the product the device forms, in fp32
                want = _mk(c.base, kind, w=wi).run(x.clone(), labels=lab, noise=Z)
                assert torch.equal(got[i], want[i]), \
                    f"{case} {kind} image {i}: max|d| {(got[i] - want[i]).abs().max().item():.3e}"
            for i, j in ((0, 1), (0, 2), (1, 2)):
                assert not torch.equal(got[i], got[j]), f"{case} {kind}: images {i} and {j} ran one weight"


def test_multipliers_come_and_go_with_the_run():
    """guidance_scale holds for the one run: the next run without it is the plain table again; a sampler without a row
    table takes multipliers of its scalar w."""
    n, m = 3, [1.0, 0.5, 0.25]
    with _Case("tail2_f32_cfg") as c:
        x = _x(1, seed=5).repeat(n, 1, 1, 1).contiguous()
        lab = torch.full((n,), 3, dtype=torch.int32, device=DEV)
        Z = _noise(x[:1], seed=19).repeat(1, n, 1, 1, 1).contiguous()
        table = _mk(c.base, guidance=[W] * K)
        got = table.run(x.clone(), labels=lab, noise=Z, guidance_scale=_f32(m))
        assert table.model.native(n).query("guidance") == 2
        plain = table.run(x.clone(), labels=lab, noise=Z)
        assert table.model.native(n).query("guidance") == 1
        assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], plain[0]) and torch.equal(plain[2], plain[0])
        assert not torch.equal(got[1], got[0])
        bare = _mk(c.base)
        assert torch.equal(bare.run(x.clone(), labels=lab, noise=Z, guidance_scale=_f32(m)), got)
        assert torch.equal(bare.run(x.clone(), labels=lab, noise=Z), plain)
        assert bare.model.native(n).query("guidance") == 0
        with pytest.raises(ValueError, match="guidance_scale has 2 entries for 3 images"):
            bare.run(x.clone(), labels=lab, noise=Z, guidance_scale=_f32(m[:2]))


# ----------------------------------------------------------------------------- 4. cond-only rows
@pytest.mark.parametrize("case", CFG_CASES)
def test_cond_only_rows(case):
    rows = [0.0, 1.8, 1.8, 0.0]
    with _Case(case) as c:
        n = c.n
        x, lab = _x(n, c.a.img_size, seed=6), _labels(n)
        Z = _noise(x)
        table = _mk(c.base, guidance=rows)
        nat = table._native(n)
        # --- skip on (shipped)
        caps = nat.query("graph_captures")
        on = table.run(x.clone(), labels=lab, noise=Z)
        assert nat.query("graph_captures") == caps + 2, "one graph for the guided program, one for the cond-only one"
        assert nat.query("cond_only_steps") == 2 and table.last_cond_only_steps == 2
        assert table.last_unet_evals_per_image == 6 == table.unet_evals_per_image()
        table.set_guidance([0.0, 0.9, 1.2, 0.0])  # new values: uploaded under the graphs already captured
        other = table.run(x.clone(), labels=lab, noise=Z)
        assert nat.query("graph_captures") == caps + 2 and not torch.equal(other, on)
        table.set_guidance(rows)
        assert torch.equal(table.run(x.clone(), labels=lab, noise=Z, graph=False), on), "eager: two resolved programs"
        assert nat.query("graph_captures") == caps + 2
        on_rows = []
        for k in range(K):
            on_rows.append(table.run(x.clone(), t_begin=k, t_end=k, labels=lab, noise=Z, clip=False))
            assert nat.query("cond_only_steps") == (1 if rows[k] == 0.0 else 0)
        # row 3 from the forward API's eps at batch n
        e = table.model(x, TAU[3], lab).double()
        r = {key: float(v[3].float()) for key, v in table.rows.items()}
        assert r["sg"] > 0.0
        xd, zd = x.double(), Z[3].double()
        x0 = (r["a0"] * xd - r["b0"] * e).clamp(-1, 1)
        want = (r["c0"] * x0 + r["cx"] * xd) + r["sg"] * zd
        bound = EPS * (abs(r["c0"]) * ((r["a0"] * xd).abs() + (r["b0"] * e).abs()) + 3 * (r["c0"] * x0).abs()
                       + 3 * (r["cx"] * xd).abs() + 2 * (r["sg"] * zd).abs())
        d = (on_rows[3].double() - want).abs()
        print(f"{case}: cond-only row 3 vs the forward: max|d| {d.max().item():.3e}, max d/bound "
              f"{(d / bound).max().item():.3f}")
        assert bool((d <= bound).all()), f"{case}: max excess {(d - bound).max().item():.3e}"
        # the traced and the 2M forms walk both kinds of row
        tr = table.new_trace(n)
        assert torch.equal(table.run(x.clone(), labels=lab, noise=Z, trace=tr), on) and torch.isfinite(tr).all()
        two_m = _mk(c.base, "dpmpp2m", guidance=rows)
        tr2 = two_m.new_trace(n)
        m_on = two_m.run(x.clone(), labels=lab, trace=tr2)
        assert two_m._native(n).query("cond_only_steps") == 2 and torch.isfinite(tr2).all()
        # --- skip off: every row on the doubled batch through the table
        rt.set_option("cfg_skip", 0)
        off = table.run(x.clone(), labels=lab, noise=Z)
        assert nat.query("cond_only_steps") == 0 and table.last_unet_evals_per_image == 8
        zero = _mk(c.base, w=0.0)
        for k in range(K):
            got = table.run(x.clone(), t_begin=k, t_end=k, labels=lab, noise=Z, clip=False)
            if k in (1, 2):
                want_k, what = on_rows[k], "the table's guided row under cfg_skip 1"
            else:
                want_k, what = zero.run(x.clone(), t_begin=k, t_end=k, labels=lab, noise=Z, clip=False), "scalar w = 0"
            assert torch.equal(got, want_k), f"{case} row {k} vs {what}: max|d| {(got - want_k).abs().max().item():.3e}"
        m_off = two_m.run(x.clone(), labels=lab)
        rt.set_option("cfg_skip", 1)
        for name, p, q in (("ddim", on, off), ("dpmpp2m", m_on, m_off)):
            dd = p.double() - q.double()
            mx, l2 = float(dd.abs().max()), float(dd.norm() / q.double().norm())
            print(f"{case} {name}: cond-only vs doubled batch: max|d| {mx:.3e}, relative L2 {l2:.3e}")
            if c.precision == "fp32":
                assert mx <= 2e-3
            else:
                assert l2 <= 3e-2


# ----------------------------------------------------------------------------- 5. the whole loop against fp64
ROWS5, M5 = [0.0, 1.8, 0.9, 0.0], [1.0, 0.5]


@pytest.fixture(scope="module")
def oracle_run():
    """The x0-form loop in fp64 around oracle.ref_cpu's UNet (test_gpu_sampler_x0.py's _oracle_loop) with
    e = (1 + w_ki) eps_c - w_ki eps_u, w_ki = w_rows[k] m_i formed from the fp32 operands."""
    a = TINY_CFG
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 32, 32, generator=g)
    Z = torch.randn(K, 2, 3, 32, 32, generator=g)
    lab = torch.tensor([3, 7])
    rows = _mk(_sampler(a)).rows
    sd = {k: v.double() for k, v in synthetic_state_dict(a, 0).items()}

    def net(xx, tt, ll):
        return R.unet_forward(sd, xx, tt, a.ch, a.ch_mult, a.attn, a.num_res_blocks, labels=ll, cfg=True)

    m = _f32(M5).double().view(2, 1, 1, 1)
    xs = x.double()
    with torch.no_grad():
        for k in range(K - 1, -1, -1):
            t = torch.full((2,), TAU[k], dtype=torch.long)
            w = float(_f32(ROWS5[k])) * m
            e = (1.0 + w) * net(xs, t, lab) - w * net(xs, t, torch.zeros_like(lab))
            x0 = (rows["a0"][k] * xs - rows["b0"][k] * e).clamp(-1, 1)
            xs = rows["c0"][k] * x0 + rows["cx"][k] * xs + rows["sg"][k] * Z[k].double()
    return x, Z, lab, xs.clamp(-1, 1)


@pytest.mark.parametrize("case", ["tail2_f32_cfg", "tail_mfma_cfg"])
def test_whole_loop_vs_oracle(oracle_run, case):
    x, Z, lab, want = oracle_run
    with _Case(case) as c:
        s = _mk(c.base, guidance=ROWS5)
        got = s.run(x.to(DEV).clone(), labels=lab.to(DEV).int(), noise=Z.to(DEV), guidance_scale=_f32(M5))
        assert s.model.native(2).query("cond_only_steps") == 2
        d = got.cpu().double() - want
        mx, l2 = float(d.abs().max()), float(d.norm() / want.norm())
        print(f"{case}: max|d| {mx:.3e}, relative L2 {l2:.3e}")
        if c.precision == "fp32":
            assert mx <= 2e-3
        else:
            assert l2 <= 3e-2


# ----------------------------------------------------------------------------- 6. refusals and lifetime
def _refused(fn, *words):
    with pytest.raises(rt.ItsdError) as ei:
        fn()
    assert ei.value.code == rt.ITSD_ERR_INVALID
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_refusals_and_lifetime():
    base = _sampler(TINY_CFG)  # ancestral, its own handle
    n = 2
    x, lab = _x(n, seed=8), _labels(n)
    Z = _noise(x)
    before = base.run(x.clone(), labels=lab, seed=SEED)
    nat = base._native(n)
    rows = _f32([0.0, 1.8, 1.8, 0.0])
    # the ancestral form is out (T_sched = 12 rows would not be refused for their count: the form is)
    _refused(lambda: nat.set_guidance(torch.ones(T)), "itsd_set_guidance", "no x0-form schedule")
    s = _mk(base, guidance=rows)
    got = s.run(x.clone(), labels=lab, noise=Z)
    assert s._native(n) is nat and nat.query("guidance") == 1 and nat.query("sched_form") == 1
    _refused(lambda: nat.set_guidance(torch.ones(K + 1)), "itsd_set_guidance", "rows = 5 != T_sched = 4")
    _refused(lambda: nat.set_guidance(torch.ones(K - 1)), "itsd_set_guidance", "rows = 3")
    _refused(lambda: nat.set_guidance(rows, torch.ones(nat.max_batch + 1)), "itsd_set_guidance", "n_img")
    assert rt.lib().itsd_set_guidance(nat.h, rows.data_ptr(), K, rows.data_ptr(), 0) == rt.ITSD_ERR_INVALID
    assert "n_img = 0" in rt.lib().itsd_last_error().decode()
    for bad in (float("nan"), float("inf"), -float("inf")):
        r = rows.clone()
        r[2] = bad
        _refused(lambda: nat.set_guidance(r), "itsd_set_guidance", "w_rows[2] is not finite")
        _refused(lambda: nat.set_guidance(rows, _f32([1.0, bad])), "itsd_set_guidance", "w_img[1] is not finite")
    # a refused call leaves the installed table in place
    assert nat.query("guidance") == 1 and torch.equal(s.run(x.clone(), labels=lab, noise=Z), got)
    # per-image multipliers: a larger batch is refused at the run, and so is predict_x0
    nat.set_guidance(rows, _f32([1.0]))
    assert nat.query("guidance") == 2
    _refused(lambda: nat.run(x.clone(), K - 1, 0, 0, noise=Z, labels=lab), "itsd_sampler_run", "per-image guidance")
    _refused(lambda: s.predict_x0(x, 2, labels=lab), "itsd_sampler_predict_x0", "per-image")
    # rows only: predict_x0 guides with the row's weight as its scalar
    nat.set_guidance(rows)
    for k in (1, 3):
        want = _mk(base, w=float(rows[k])).predict_x0(x, k, labels=lab)
        s._native(n)  # (the scalar sampler's schedule install detached the table: s puts both back)
        assert nat.query("guidance") == 1
        assert torch.equal(s.predict_x0(x, k, labels=lab), want), f"predict_x0 at row {k}"
    # detach by hand, and by installing a schedule
    nat.set_guidance(None, None)
    assert nat.query("guidance") == 0
    nat._guidance = None  # (what the handle now holds)
    assert torch.equal(s.run(x.clone(), labels=lab, noise=Z), got) and nat.query("guidance") == 1
    after = base.run(x.clone(), labels=lab, seed=SEED)  # the ancestral sampler on the same handle
    assert base._native(n) is nat and nat.query("guidance") == 0 and nat.query("sched_form") == 0
    assert torch.equal(before, after)
    assert torch.equal(s.run(x.clone(), labels=lab, noise=Z), got) and nat.query("guidance") == 1
    # the Python surface
    with pytest.raises(ValueError, match="guidance= needs sampler"):
        CondGaussianDiffusionSampler(base.model, 1e-4, 0.028, T, w=W, guidance=[W] * T)
    with pytest.raises(ValueError, match="guidance has 3 rows"):
        _mk(base, guidance=[W] * 3)
    with pytest.raises(ValueError, match="guidance_scale needs sampler"):
        base.run(x.clone(), labels=lab, seed=SEED, guidance_scale=_f32([1.0, 1.0]))


def test_non_cfg_handle_is_refused():
    plain = _sampler(ARCH_TINY)
    ddim = type(plain)(plain.model, plain.sched.beta_1, plain.sched.beta_T, T, sampler="ddim", steps=K)
    x = _x(2, seed=9)
    ddim.run(x.clone(), seed=SEED)
    _refused(lambda: ddim._native(2).set_guidance(torch.ones(K)), "itsd_set_guidance", "not a CFG UNet")
    with pytest.raises(ValueError, match="guidance_scale belongs to the conditional sampler"):
        ddim.run(x.clone(), seed=SEED, guidance_scale=_f32([1.0, 1.0]))
    with pytest.raises(ValueError, match="guidance= belongs to the conditional sampler"):
        type(plain)(plain.model, 1e-4, 0.02, T, sampler="ddim", steps=K, guidance=[1.0] * K)


# ----------------------------------------------------------------------------- 7. one search
def test_random_search_over_guidance_scales(tmp_path):
    scales, n_cand, shape = [0.5, 1.0], 4, (1, 3, 32, 32)
    base = _sampler(TINY_CFG)
    s = _mk(base, guidance=guidance_rows(TAU, W, {"kind": "interval", "t_lo": 5, "t_hi": 8}))
    lab = torch.tensor([4], dtype=torch.int32, device=DEV)
    ver = OracleVerifier()
    eng = SearchEngine(s, ver, seed=5, guidance_scales=scales)
    best, score, h = eng.random_search(n_cand, shape, labels=lab)
    # the round by hand
    x = eng.candidate_noise(0, 0, n_cand, shape)
    s.run(x, labels=lab.repeat(n_cand), seed=(5 * 1000003) & MASK62, noise_offset=0,
          guidance_scale=_f32([0.5, 1.0, 0.5, 1.0]))
    sc = ver.score_batch(x, n_cand).cpu()
    assert h["scores"] == sc.tolist() and score == float(sc.max())
    bi = h["best_index"]
    assert bi == int(sc.argmax()) and torch.equal(eng.best_image, x[bi:bi + 1])
    assert h["guidance_scales"] == [0.5, 1.0, 0.5, 1.0] and h["best_guidance_scale"] == scales[bi % 2]
    assert torch.equal(best, eng.candidate_noise(0, bi, 1, shape))
    # the scales act: candidate 0 alone under scale 1.0 is another image
    y = eng.candidate_noise(0, 0, 1, shape)
    s.run(y, labels=lab, seed=(5 * 1000003) & MASK62, noise_offset=0, guidance_scale=_f32([1.0]))
    assert not torch.equal(y[0], x[0])
    assert s.last_unet_evals_per_image == 6
    # the entry point: MainCondition's surface with a guidance block and search.guidance_scales
    sd = synthetic_state_dict(TINY_CFG, 6)
    torch.save(sd, str(tmp_path / "ckpt_63_.pt"))
    cfg = E.load_config(None, [f"save_dir={tmp_path}", "test_load_weight=ckpt_63_.pt", "T=12", "channel=32",
                               "channel_mult=[1,2]", "num_res_blocks=1", "batch_size=10", f"sampled_dir={tmp_path}",
                               "seed=1", "sampler.kind=ddim", "sampler.steps=4", "sampler.eta=0.5",
                               "sampler.clip_x0=true", "guidance.kind=interval", "guidance.t_lo=5", "guidance.t_hi=8",
                               "search.algorithm=random", "search.n_candidates=4", "search.guidance_scales=[0.5,1.0]"],
                        config_name="condition_config")
    res = E.run(cfg, condition=True)
    with open(tmp_path / "SearchBestImgs.json") as fh:
        js = json.load(fh)
    assert js["unet_evals_per_image"] == 6 and res["unet_evals_per_image"] == 6
    assert js["history"]["guidance_scales"] == [0.5, 1.0, 0.5, 1.0]
    assert js["history"]["best_guidance_scale"] == scales[js["history"]["best_index"] % 2]
    assert res["search"]["history"] == js["history"]
    # the same eval by hand: the table sampler called directly
    torch.manual_seed(1)
    net = CondUNet(12, 10, 32, [1, 2], 1, 0.0).to(DEV)
    net.load_state_dict(sd)
    xe = torch.randn(10, 3, 32, 32, device=DEV)
    hand = CondGaussianDiffusionSampler(net, 1e-4, 0.028, 12, w=1.8, sampler="ddim", steps=4, eta=0.5, clip_x0=True,
                                        guidance=_f32([0.0, 1.8, 1.8, 0.0]))
    assert torch.equal(hand(xe, res["labels"]) * 0.5 + 0.5, res["sampled"])
