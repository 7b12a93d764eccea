"""GPU tests of the model-as-verifier: the probe noising kernel, the sse epilogue of every tail kernel
(TailArgs::step_mode 4, itsd_verify_denoise) and DenoisingVerifier in the search engine. Tiny UNets with seeded synthetic
weights, T = 12; the six tail forms are TAIL_CASES of test_gpu_path_branch.py, whose docstring names the kernel each
one runs. The weights are synthetic: nothing here says the score prefers better images, the checks pin mechanics.

The probe is, in fp32 with contraction off,
    x_t = (a x0) + (b z);   d = z - eps;   q = d d;   sse = sum_e q
with z ONE field for the whole batch, indexed by the element within the image. x_t is bit equality against torch.

The bound of check 2, |sse - ref| <= (4 + L) 2^-24 ref with ref = sum_e (double(z) - double(eps))^2 over the call's own
eps_out, is derived, not measured. u = 2^-24 is the unit roundoff. z and eps are fp32 values, exact in fp64; d carries
one rounding and enters q twice, the square rounds once: q = q_exact (1 + 3u) to first order. Every q is >= 0, so a
chain of L fp32 additions over them keeps a relative error of L u, and the fp64 finalize adds nothing at this scale;
one more u covers every second-order term ((3 + L)^2 u^2 / 2 < 2^-40). L, the longest chain of fp32 additions an
element passes through: the thread's own items, the 6-level lane butterfly, the wave partials in
wave order:
    tail2_kernel       1 item a thread (0 + q is exact)        0 + 6 + 3 (4 waves)  =  9
    tail_kernel        3 items a thread                        2 + 6 + 3 (4 waves)  = 11
    tail_mfma_kernel   1 item a thread                         0 + 6 + 7 (8 waves)  = 13
"""
import pytest
import torch

from itsd import runtime as rt
from itsd.arch import ARCH_TINY
from itsd.diffusion import CondGaussianDiffusionSampler, GaussianDiffusionSampler
from itsd.search import SearchEngine, rank_desc, strict_argmax
from itsd.schedule import renoise_coeffs
from itsd.verifier import DenoisingVerifier, OracleVerifier, combine_sse
from itsd.weights import synthetic_state_dict
from test_gpu_path_branch import DEV, MASK62, TAIL_CASES, TINY_CFG, T, _f32, _net, _sampler, _x

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
L_CHAIN = {"tail2_f32": 9, "tail_mfma": 13, "tail2_bf16": 9, "tail_f32_cfg_128px": 11, "tail2_f32_cfg": 9,
           "tail_mfma_cfg": 13}
ROW = 5
SEED, SID = 0x5EED, 0xD0000001
SHAPE = (1, 3, 32, 32)


def _ab(smp, row=ROW):
    abar = smp.abar_rows.double()[row]
    return _f32(float(torch.sqrt(abar))), _f32(float(torch.sqrt(1.0 - abar)))


def _labels(a, n):
    return torch.tensor([3, 7, 1], dtype=torch.int32, device=DEV)[:n] if a.cfg else None


def _field(img, seed=SEED, sid=SID):
    """The probe's Philox field: itsd_noise's draw for ONE candidate of 3 H W elements."""
    return rt.noise(torch.empty(1, 3, img, img, device=DEV), 1, seed, sid)[0]


def _probe(smp, x0, lab, noise=None, row=ROW, debug=True, seed=SEED, sid=SID):
    """One itsd_verify_denoise call: (sse [n, 2], x_t, eps_out [1 or 2, n, 3, H, W])."""
    n = x0.shape[0]
    a, b = _ab(smp, row)
    nat = smp._native(n)
    xt = torch.full_like(x0, float("nan")) if debug else None
    eps = torch.full((2 if smp.model.arch.cfg else 1,) + tuple(x0.shape), float("nan"), device=DEV) if debug else None
    sse = torch.full((n, 2), float("nan"), dtype=torch.float64, device=DEV)
    nat.verify_denoise(x0, row, a, b, seed, sid, labels=lab, noise=noise, sse=sse, xt_out=xt, eps_out=eps)
    return sse, xt, eps


def _ref_sse(z, eps):
    """sum_e (double(z) - double(eps))^2 per image and branch: [n, branches]."""
    d = z.double()[None, None] - eps.double()
    return (d * d).flatten(2).sum(dim=2).t()


def _check_bound(tag, sse, ref, L):
    branches = ref.shape[1]
    err = (sse[:, :branches] - ref).abs()
    ratio = float((err / ((4 + L) * U * ref)).max())
    print(f"{tag}: max |sse - ref| / ((4 + {L}) u ref) = {ratio:.3f}; sse {sse[:, :branches].flatten().tolist()}")
    assert bool((ref > 0).all()) and bool(torch.isfinite(sse).all())
    assert bool((err <= (4 + L) * U * ref).all()), f"{tag}: ratio {ratio:.3f}"
    if branches == 1:
        assert bool((sse[:, 1] == 0).all()), f"{tag}: DDPM computes no second error"


_FORMS = {}


def _forms(case):
    """Every call checks 1-3 compare for one tail form, made once inside its io_mfma window."""
    if case in _FORMS:
        return _FORMS[case]
    a, precision, io_mfma, n = TAIL_CASES[case]
    rt.set_option("io_mfma", io_mfma)
    try:
        smp = _sampler(a, precision)
        x0, lab = _x(n, a.img_size, seed=3).clamp(-1, 1), _labels(a, n)
        keep = x0.clone()
        r = {"x0": x0, "n": n, "ab": _ab(smp), "cfg": a.cfg}
        r["z"] = _field(a.img_size)
        r["philox"] = _probe(smp, x0, lab)
        r["zi"] = torch.randn(3, a.img_size, a.img_size, generator=torch.Generator().manual_seed(17)).to(DEV)
        r["injected"] = _probe(smp, x0, lab, noise=r["zi"])
        assert torch.equal(x0, keep), "the probe modified x0"
        xt = r["philox"][1]
        if a.cfg:
            r["model"] = torch.stack([smp.model(xt, ROW, lab), smp.model(xt, ROW, torch.zeros_like(lab))])
        else:
            r["model"] = smp.model(xt, ROW)[None]
    finally:
        rt.set_option("io_mfma", 1)
    _FORMS[case] = r
    return r


# ----------------------------------------------------------------------------- 1. x_t bits
@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_xt_bits(case):
    r = _forms(case)
    a, b = r["ab"]
    for key, z in (("philox", r["z"]), ("injected", r["zi"])):
        want = (a * r["x0"]) + (b * z)[None]
        got = r[key][1]
        assert torch.equal(got, want), f"{case} {key}: max|d| {(got - want).abs().max().item():.3e}"
    assert not torch.equal(r["philox"][1], r["injected"][1])


# ----------------------------------------------------------------------------- 2. sse against fp64, every tail form
@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_sse_vs_fp64(case):
    r = _forms(case)
    for key, z in (("philox", r["z"]), ("injected", r["zi"])):
        sse, _, eps = r[key]
        assert bool(torch.isfinite(eps).all())
        _check_bound(f"{case} {key}", sse, _ref_sse(z, eps), L_CHAIN[case])


# ----------------------------------------------------------------------------- 3. eps_out is the model's, unguided
@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_eps_is_the_models(case):
    """eps_out against the forward API on the probe's own x_t: DESIGN section 4's per-forward bounds (fp32 max-abs
    <= 2e-4, bf16 relative L2 <= 2e-2). DDPM: the forward at equal n runs the same kernels, so the bits are equal.
    CFG (w = 1.8): the two branches are the model under the label and under label 0, apart -- not the guided eps."""
    r = _forms(case)
    eps, want = r["philox"][2], r["model"]
    precision = TAIL_CASES[case][1]
    for k in range(eps.shape[0]):
        d = eps[k].double() - want[k].double()
        mx, l2 = float(d.abs().max()), float(d.norm() / want[k].double().norm())
        print(f"{case} branch {k}: max|d| {mx:.3e}, relative L2 {l2:.3e}")
        if precision == "fp32":
            assert mx <= 2e-4
        else:
            assert l2 <= 2e-2
    if not r["cfg"]:
        assert torch.equal(eps, want), f"{case}: the probe's eps is not the forward's bit for bit"
    else:
        assert not torch.equal(eps[0], eps[1]), f"{case}: the two branches are one"
        guided = 2.8 * want[0].double() - 1.8 * want[1].double()
        assert float((eps[0].double() - guided).abs().max()) > 10 * float((eps[0] - want[0]).abs().max())


# ----------------------------------------------------------------------------- 4. the tail's draw is the noising kernel's
@pytest.mark.parametrize("case", ["tail2_f32", "tail_mfma", "tail_f32_cfg_128px"])
def test_zero_tail_gives_the_sum_of_z_squared(case):
    """A tail conv of zero weight and bias makes eps == 0, so sse[:, 0] (and CFG's sse[:, 1]) = sum_e z[e]^2, the same
    for every image: an index that is not the element within the image (the batch offset, say) fails for image >= 1."""
    a, precision, io_mfma, n = TAIL_CASES[case]
    sd = synthetic_state_dict(a, 0)
    sd["tail.2.weight"].zero_()
    sd["tail.2.bias"].zero_()
    rt.set_option("io_mfma", io_mfma)
    try:
        net = _net(a, precision)
        net.load_state_dict(sd)
        smp = (CondGaussianDiffusionSampler(net, 1e-4, 0.028, T, w=1.8) if a.cfg
               else GaussianDiffusionSampler(net, 1e-4, 0.02, T))
        x0, lab = _x(n, a.img_size, seed=4), _labels(a, n)
        z = _field(a.img_size)
        zi = torch.randn(3, a.img_size, a.img_size, generator=torch.Generator().manual_seed(23)).to(DEV)
        got = {"philox": (_probe(smp, x0, lab), z), "injected": (_probe(smp, x0, lab, noise=zi), zi)}
    finally:
        rt.set_option("io_mfma", 1)
    for key, ((sse, _, eps), field) in got.items():
        assert float(eps.abs().max()) == 0.0
        ref = (field.double() ** 2).sum().expand(n, eps.shape[0])
        _check_bound(f"{case} zero tail {key}", sse, ref, L_CHAIN[case])
        assert bool((sse[:, :eps.shape[0]] == sse[0, 0]).all()), f"{case} {key}: images disagree {sse.tolist()}"


# ----------------------------------------------------------------------------- 5. a pure function of the image
def _plans(nat, n):
    return [{k: v for k, v in nat.op_info(n, op, step=True).items()} for op in range(nat.query("ops") + 2)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_score_is_a_function_of_the_image(precision):
    """Three distinct images scored together, in reversed order, and each alone (n = 1), on one handle: bit-equal per
    image. fp32: asserted outright. bf16 (where test_gpu_parity.py asserts trajectories batch-invariant, ARCH_TINY at
    32 px, a batch of 8 against its second half): the batch of 8 against its second half is asserted bit-equal here
    too, and the reversed order always; n = 1 against n = 3 is asserted bit-equal when the step program resolves to
    the same launches at both batches (itsd_unet_op_info), else each call is held to check 2's bound -- the test
    prints which."""
    smp = _sampler(ARCH_TINY, precision)
    L = L_CHAIN["tail2_f32" if precision == "fp32" else "tail_mfma"]
    x0 = _x(3, seed=8).clamp(-1, 1)
    z = _field(32)
    s3, _, e3 = _probe(smp, x0, None)
    _check_bound(f"{precision} n=3", s3, _ref_sse(z, e3), L)
    assert len({float(v) for v in s3[:, 0]}) == 3
    rev, _, _ = _probe(smp, x0.flip(0).contiguous(), None)
    assert torch.equal(rev.flip(0), s3), f"{precision}: order changed the sums {s3.tolist()} {rev.tolist()}"
    nat = smp._native(3)
    same_plan = _plans(nat, 1) == _plans(nat, 3)
    print(f"{precision}: step program at n = 1 {'==' if same_plan else '!='} at n = 3")
    for i in range(3):
        s1, _, e1 = _probe(smp, x0[i:i + 1].contiguous(), None)
        _check_bound(f"{precision} image {i} alone", s1, _ref_sse(z, e1), L)
        if precision == "fp32" or same_plan:
            assert torch.equal(s1[0], s3[i]), f"{precision} image {i}: alone {s1.tolist()} in the batch {s3[i].tolist()}"
    x8 = _x(8, seed=9).clamp(-1, 1)
    full, _, _ = _probe(smp, x8, None, debug=False)
    half, _, _ = _probe(smp, x8[4:].contiguous(), None, debug=False)
    assert torch.equal(full[4:], half), f"{precision}: the second half of 8 scored apart differs"
    # another seed or stream id is another field
    other, _, _ = _probe(smp, x0, None, debug=False, sid=SID + 1)
    assert not torch.equal(other, s3)


# ----------------------------------------------------------------------------- 6. poison
@pytest.mark.parametrize("arch", ["ddpm", "cfg"])
def test_poison_and_isolation(arch):
    """After itsd_unet_poison (which also fills the probe's own two buffers) the call gives the bits it gave before:
    no launch of the probe reads what no launch of it wrote. No graph is captured, the hand-off status is 0, and a
    sampler run after a probe is the run without it. (The NaN flag has no reader of its own in the ABI: run_begin
    resets it, so what is observable is that the run reports no NaN.)"""
    a = TINY_CFG if arch == "cfg" else ARCH_TINY
    smp = _sampler(a, "bf16")
    n = 2
    x0, lab = _x(n, seed=6).clamp(-1, 1), _labels(a, n)
    xT = _x(n, seed=7)
    run0 = smp.run(xT.clone(), labels=lab, seed=11)
    nat = smp._native(n)
    caps = nat.query("graph_captures")
    first = _probe(smp, x0, lab)
    nat.poison(DEV)
    second = _probe(smp, x0, lab)
    for p, q in zip(first, second):
        assert bool(torch.isfinite(q).all()) and torch.equal(p, q)
    assert nat.query("status") == 0 and nat.query("graph_captures") == caps
    run1 = smp.run(xT.clone(), labels=lab, seed=11)
    assert torch.equal(run0, run1) and nat.query("graph_captures") == caps
    third = _probe(smp, x0, lab)
    assert torch.equal(third[0], first[0])


# ----------------------------------------------------------------------------- 7. validation
def test_refusals():
    L = rt.lib()
    smp, cond = _sampler(ARCH_TINY), _sampler(TINY_CFG)
    x0 = _x(2, seed=1)
    sse = torch.empty(2, 2, dtype=torch.float64, device=DEV)
    lab = _labels(TINY_CFG, 2)

    def call(nat, x=x0.data_ptr(), labels=None, n=2, t=ROW, out=sse.data_ptr()):
        rc = L.itsd_verify_denoise(nat.h, x, labels, n, t, 0.8, 0.6, 1, 2, None, out, None, None, rt.stream_ptr(DEV))
        return rc, L.itsd_last_error().decode()

    nat = smp._native(2)
    cap = nat.query("max_batch")
    for kw in (dict(x=None), dict(out=None), dict(n=0), dict(n=cap + 1), dict(t=-1), dict(t=T)):
        rc, msg = call(nat, **kw)
        assert rc == rt.ITSD_ERR_INVALID and msg, kw
    assert call(nat)[0] == rt.ITSD_OK
    cnat = cond._native(2)
    rc, msg = call(cnat)
    assert rc == rt.ITSD_ERR_INVALID and "labels" in msg
    assert call(cnat, labels=lab.data_ptr())[0] == rt.ITSD_OK
    rc, msg = L.itsd_verify_denoise(None, x0.data_ptr(), None, 2, ROW, 0.8, 0.6, 1, 2, None, sse.data_ptr(), None,
                                    None, None), L.itsd_last_error().decode()
    assert rc == rt.ITSD_ERR_INVALID and msg
    bare = _net(ARCH_TINY).native(2)  # no schedule installed
    rc, msg = call(bare)
    assert rc == rt.ITSD_ERR_INVALID and "schedule" in msg
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="class"):
        DenoisingVerifier(smp, mode="class")
    with pytest.raises(ValueError, match="labels"):
        DenoisingVerifier(cond, mode="class").score_batch(x0, 2)


# ----------------------------------------------------------------------------- 8. the engine
def _by_hand(ver, images, n, lab):
    """The verifier applied by hand: its probes through the ABI binding, combined in fp64."""
    smp = ver.sampler
    nat = smp._native(images.shape[0])
    sse = torch.stack([nat.verify_denoise(images, row, a, b, ver.seed, 0xD0000000 + r, labels=lab)
                       for r, (row, (a, b)) in enumerate(zip(ver.rows, ver.ab))])
    return combine_sse(sse, ver.mode, images[0].numel(), n).cpu()


@pytest.fixture(scope="module")
def smp_cfg():
    return _sampler(TINY_CFG)


def test_engine_random_round_class_verifier(smp_cfg):
    n, seed = 4, 6
    lab1 = torch.tensor([4], dtype=torch.int32, device=DEV)
    lab = lab1.repeat(n)
    oracle = SearchEngine(smp_cfg, OracleVerifier(), seed=seed)
    ob, os_, oh = oracle.random_search(n, SHAPE, labels=lab1)
    oimg = oracle.best_image.clone()
    ver = DenoisingVerifier(smp_cfg, mode="class", probes=2)
    assert ver.rows == [3, 9] and ver.probes == 2
    eng = SearchEngine(smp_cfg, ver, seed=seed)
    _, score, h = eng.random_search(n, SHAPE, labels=lab1)
    x = eng.candidate_noise(0, 0, n, SHAPE)
    smp_cfg.run(x, labels=lab, seed=(seed * 1000003) & MASK62, noise_offset=0)
    want = _by_hand(ver, x, n, lab)
    assert torch.equal(torch.tensor(h["scores"], dtype=torch.float64), want), f"{h['scores']} {want.tolist()}"
    assert bool(torch.isfinite(want).all()) and len(set(want.tolist())) == n
    bi, bs = strict_argmax(want)
    assert h["best_index"] == bi and score == bs and h["verifier_unet_steps"] == n * 2
    assert torch.equal(eng.best_image, x[bi:bi + 1])
    one = ver.score(x[bi:bi + 1], labels=lab1)  # the one-candidate form
    assert one == float(ver.score_batch(x[bi:bi + 1], 1, labels=lab1)[0]) and one == ver(x[bi:bi + 1], labels=lab1)
    # another label is another score: the verifier sees the label
    assert not torch.equal(ver.score_batch(x, n, labels=torch.full_like(lab, 7)).cpu(), want)
    ab, as_, ah = oracle.random_search(n, SHAPE, labels=lab1)
    assert ah == oh and as_ == os_ and torch.equal(ab, ob) and torch.equal(oracle.best_image, oimg)
    assert "verifier_unet_steps" not in oh


def test_engine_branching_round_class_verifier(smp_cfg):
    n, seed, steps, keep, delta = 4, 6, [6], 2, 2
    lab1 = torch.tensor([4], dtype=torch.int32, device=DEV)
    lab = lab1.repeat(n)
    oracle = SearchEngine(smp_cfg, OracleVerifier(), seed=seed)
    init = oracle.initial_noise(SHAPE)
    ob, os_, oh = oracle.path_search_branch(init, n, 0.5, steps, keep=keep, renoise_steps=delta, labels=lab1)
    ver = DenoisingVerifier(smp_cfg, mode="class", probes=2)
    eng = SearchEngine(smp_cfg, ver, seed=seed)
    best, score, h = eng.path_search_branch(init, n, 0.5, steps, keep=keep, renoise_steps=delta, labels=lab1)
    # by hand (the parts test_gpu_path_branch.py documents), the verifier on the stage's x0 estimate
    key = lambda i: (seed * 1000003 + (0x5B000000 + i if (i and delta) else 0)) & MASK62  # noqa: E731
    x = eng.candidate_noise(0, 0, n, SHAPE, init, 0.5)
    s = steps[0]
    smp_cfg.run(x, t_begin=T - 1, t_end=s + 1, labels=lab, seed=key(0), noise_offset=0, clip=False)
    sc0 = _by_hand(ver, smp_cfg.predict_x0(x, s, labels=lab), n, lab)
    order, m = rank_desc(sc0), n // keep
    tab = [order[j // m] for j in range(n)]
    a, b = renoise_coeffs(smp_cfg.sched.alphas_bar, s, delta)
    x = rt.branch(torch.empty_like(x), x, tab, a, b, seed, 0xC0000000, cand_offset=0)
    smp_cfg.run(x, t_begin=s + delta, t_end=0, labels=lab, seed=key(1), noise_offset=0, clip=True)
    sc = _by_hand(ver, x, n, lab)
    assert h["stage_scores"] == [sc0.tolist()] and h["parents"] == [tab] and h["scores"] == sc.tolist()
    bi, bs = strict_argmax(sc)
    assert h["best_index"] == bi and score == bs and torch.equal(eng.best_image, x[bi:bi + 1])
    assert h["verifier_unet_steps"] == 2 * n * 2 and h["unet_steps"] == n * ((5 + 9) + 1)
    ab, as_, ah = oracle.path_search_branch(init, n, 0.5, steps, keep=keep, renoise_steps=delta, labels=lab1)
    assert ah == oh and as_ == os_ and torch.equal(ab, ob)


def test_entry_search_verifier_denoise(tmp_path):
    """search.verifier: denoise with verifier_probes / verifier_seed through the eval entry is the engine's own call."""
    from itsd import entry as E
    from itsd.model import UNet

    sd = synthetic_state_dict(ARCH_TINY, 5)
    torch.save(sd, str(tmp_path / "ckpt_0_.pt"))
    over = [f"save_weight_dir={tmp_path}", "test_load_weight=ckpt_0_.pt", "T=1000", f"inference_T={T}", "channel=32",
            "channel_mult=[1,2]", "attn=[1]", "num_res_blocks=1", "batch_size=2", "nrow=2", "seed=3",
            f"sampled_dir={tmp_path / 'out'}", "search.algorithm=random", "search.n_candidates=4",
            "search.verifier=denoise", "search.verifier_probes=2", "search.verifier_seed=5"]
    s = E.run(E.load_config(None, over))["search"]
    net = UNet(1000, 32, [1, 2], [1], 1, 0.0).to(DEV)
    net.load_state_dict(sd)
    smp = GaussianDiffusionSampler(net, 1e-4, 0.02, T)
    eng = SearchEngine(smp, DenoisingVerifier(smp, mode="denoise", probes=2, seed=5), seed=3)
    _, score, h = eng.random_search(4, SHAPE)
    assert s["history"] == h and s["best_score"] == score and h["verifier_unet_steps"] == 8
    assert torch.equal(s["best_image"], eng.best_image)
    with pytest.raises(ValueError, match="search.verifier"):
        E.run(E.load_config(None, [o.replace("=denoise", "=class") for o in over]))


def test_denoise_mode_under_the_few_step_sampler():
    """mode="denoise" on an unconditional model, rows of a K = 4 ddim schedule (tau = 2, 5, 8, 11): the probe at row k
    is the ancestral handle's probe at timestep tau[k] with the same a, b."""
    base = _sampler(ARCH_TINY)
    x = _x(3, seed=12).clamp(-1, 1)
    want = []
    for t in (2, 5, 8, 11):
        want.append(_probe(base, x, None, row=t, debug=False, sid=0xD0000000 + len(want))[0])
    few = GaussianDiffusionSampler(base.model, 1e-4, 0.02, T, sampler="ddim", steps=4, eta=0.0, clip_x0=True)
    ver = DenoisingVerifier(few, mode="denoise", probes=4, seed=SEED)
    assert ver.rows == [0, 1, 2, 3]
    got = ver.score_batch(x, 3)
    assert torch.equal(got, combine_sse(torch.stack(want), "denoise", x[0].numel(), 3))
    assert bool((got < 0).all()) and got.dtype == torch.float64
