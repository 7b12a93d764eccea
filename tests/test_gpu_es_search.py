"""GPU tests of the gradient search without autograd: itsd_es_candidates, itsd_es_step (es_grad_kernel, es_adam_kernel,
es_norm_finalize_kernel), SearchEngine.gradient_search against its parts, and the entry point. Tiny shapes; tiny UNets
with seeded synthetic weights, T = 12 (nothing here says the search finds better images: the checks pin mechanics).

The device draw z_p is read back with itsd_noise(pivot=None, scale=1, count=1, cand_offset=p): 0 + 1 z is z exactly.
u = 2^-24 is the unit roundoff of fp32.

Candidates: bit equality with torch's fp32 pivot + (s * z) (two roundings, no contraction on either side).

Gradient: g = sum over slices of 16 pairs of (sum over the slice's pairs of (w_p z_p)), both ascending from 0. An element
passes one rounding for its product, at most min(M, 16) additions inside its slice and ceil(M / 16) across the slices;
every partial sum is bounded by S = sum_p |w_p z_p[e]|, so |g - ref| <= (min(M, 16) + ceil(M / 16) + 1) u S against
ref = sum_p w_p z_p in fp64 -- derived, not measured.

Adam: m', v' are products and sums of fp32 values in a stated order: bit equality with torch's fp32 restatement from the
read-back g. theta' = theta - ((c1 m') / ((sqrt(v') c2) + eps)) has five operations of at most one ulp each on the step
(sqrt, two products, the sum, the quotient: each moves the step by at most 2 u relative) and the final subtraction
(u |theta'|): |theta' - ref| <= u |theta'| + 10 u |step| against the fp64 value from the read-back m', v'."""
import json
import math
import os

import pytest
import torch

from itsd import entry as E
from itsd import runtime as rt
from itsd.arch import ARCH_TINY
from itsd.diffusion import GaussianDiffusionSampler
from itsd.model import UNet
from itsd.schedule import adam_coeffs
from itsd.search import GradientBasedSearch, SearchEngine, es_weights, strict_argmax
from itsd.verifier import DenoisingVerifier, OracleVerifier
from itsd.weights import synthetic_state_dict
from test_gpu_path_branch import DEV, MASK62, TINY_CFG, T, _f32, _sampler

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED, SID = 0x5EED, 0xB0000001
PERS = [75, 1027, 3072]  # scalar (odd), scalar over more than one block of the update, the 16-byte path
SHAPE = (1, 3, 32, 32)
SIGMA = _f32(0.1)


def _z(p, per, seed=SEED, sid=SID):
    return rt.noise(torch.empty(1, per, device=DEV), 1, seed, sid, cand_offset=p)[0]


def _zs(n_pairs, per, seed=SEED, sid=SID):
    """z_p for p < n_pairs: itsd_noise's candidates 0..n_pairs-1, [n_pairs, per]."""
    return rt.noise(torch.empty(n_pairs, per, device=DEV), n_pairs, seed, sid)


def _rand(per, seed, scale=1.0):
    return (torch.randn(per, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _buf(n, misalign):
    """n fp32 elements of NaN; misalign: a base 4 bytes off the allocation's 16-byte alignment."""
    b = torch.full((n + 1,), float("nan"), device=DEV)
    return b[1:] if misalign else b[:n]


# ----------------------------------------------------------------------------- 1. candidates
_CANDS = {}


def _cands(per, n_cand, off, misalign=False):
    key = (per, n_cand, off, misalign)
    if key not in _CANDS:
        pivot = _buf(per, misalign)
        pivot.copy_(_rand(per, per))
        assert pivot.data_ptr() % 16 == (4 if misalign else 0)
        out = _buf(n_cand * per, misalign).view(n_cand, per)
        rt.es_candidates(out, pivot, n_cand, SIGMA, SEED, SID, cand_offset=off)
        _CANDS[key] = (out, pivot)
    return _CANDS[key]


@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("n_cand,off", [(2, 0), (5, 3), (8, 0)])
def test_candidates_bits(per, n_cand, off):
    out, pivot = _cands(per, n_cand, off)
    for j in range(n_cand):
        c = off + j
        s = -SIGMA if c & 1 else SIGMA  # (5, 3) starts on a minus candidate
        want = pivot + (s * _z(c >> 1, per))
        assert torch.equal(out[j], want), f"per={per} candidate {c}"
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("per", PERS)
def test_candidates_misaligned_pair(per):
    got, _ = _cands(per, 5, 3, misalign=True)  # both bases 4 bytes off: the scalar form, whatever per
    assert torch.equal(got, _cands(per, 5, 3)[0])


@pytest.mark.parametrize("per", PERS)
def test_candidates_are_a_function_of_the_global_index(per):
    whole, pivot = _cands(per, 8, 0)
    lo = rt.es_candidates(torch.empty(4, per, device=DEV), pivot, 4, SIGMA, SEED, SID, cand_offset=0)
    hi = rt.es_candidates(torch.empty(4, per, device=DEV), pivot, 4, SIGMA, SEED, SID, cand_offset=4)
    assert torch.equal(whole, torch.cat([lo, hi]))
    assert torch.equal(whole[3:8], _cands(per, 5, 3)[0])


# ----------------------------------------------------------------------------- 2. / 3. the step
def _step(per, w, k=1, lr=0.01, theta=None, m=None, v=None, seed=SEED, sid=SID, grad=True):
    """One itsd_es_step on copies: (theta', m', v', g, gnorm2 [1] fp64, the fp32-cast constants)."""
    n_pairs = w.numel()
    theta = (_rand(per, 1, 1.3).clamp(-4, 4) if theta is None else theta).clone()
    m = torch.zeros(per, device=DEV) if m is None else m.clone()
    v = torch.zeros(per, device=DEV) if v is None else v.clone()
    ws = torch.full((rt.es_workspace_bytes(n_pairs, per),), 0xFF, dtype=torch.uint8, device=DEV)  # NaN bits
    g = torch.full((per,), float("nan"), device=DEV) if grad else None
    a = adam_coeffs(lr, (0.9, 0.999), 1e-8, k)
    gn2 = rt.es_step(theta, m, v, w.to(DEV), seed, sid, a, ws, grad_out=g)
    return theta, m, v, g, gn2, {key: _f32(val) for key, val in a.items()}


_GRAD = {}


def _grad_case(M, per):
    if (M, per) not in _GRAD:
        w = torch.randn(M, generator=torch.Generator().manual_seed(M * 7 + per)).float()
        _GRAD[(M, per)] = (w, _step(per, w))
    return _GRAD[(M, per)]


@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("M", [1, 3, 64, 257])
def test_gradient_bound(M, per):
    w, (_, _, _, g, gn2, _) = _grad_case(M, per)
    prod = w.to(DEV).double()[:, None] * _zs(M, per).double()
    ref, S = prod.sum(dim=0), prod.abs().sum(dim=0)
    bound = (min(M, 16) + math.ceil(M / 16) + 1) * U * S
    err = (g.double() - ref).abs()
    print(f"M={M} per={per}: max |g - ref| / bound = {float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(g).all()) and bool((err <= bound).all())
    # the norm: the fp64 sum of the read-back g^2, and the same bits on a second call
    want = float(g.double().square().sum())
    assert abs(float(gn2) - want) <= 1e-12 * want
    again = _step(per, w)
    assert torch.equal(again[4], gn2) and torch.equal(again[3], g) and torch.equal(again[0], _grad_case(M, per)[1][0])


@pytest.mark.parametrize("per", PERS)
def test_gradient_one_hot_returns_the_draw(per):
    _, _, _, g, gn2, _ = _step(per, torch.tensor([0.0, 0.0, 1.0]))
    assert torch.equal(g, _z(2, per))  # 0 + (1 z) is z: pair 2's draw, and nothing of pairs 0 and 1
    assert abs(float(gn2) / float(g.double().square().sum()) - 1) <= 1e-12


@pytest.mark.parametrize("per", PERS)
def test_gradient_all_zero_weights_leave_theta(per):
    theta0 = _rand(per, 1, 1.3).clamp(-4, 4)
    theta, m, v, g, gn2, _ = _step(per, torch.zeros(5), theta=theta0)
    assert torch.equal(g, torch.zeros_like(g)) and float(gn2) == 0.0
    assert torch.equal(theta, theta0) and not bool(m.any()) and not bool(v.any())


@pytest.mark.parametrize("per", PERS)
def test_adam_moments_bits_and_theta_bound(per):
    w = torch.randn(5, generator=torch.Generator().manual_seed(per)).float()
    theta0 = _rand(per, 2, 1.3).clamp(-4, 4)
    m0, v0 = _rand(per, 3, 0.5), _rand(per, 4, 0.5).square()
    theta, m, v, g, _, a = _step(per, w, k=3, theta=theta0, m=m0, v=v0)
    gl = -g
    assert torch.equal(m, (a["beta1"] * m0) + (a["omb1"] * gl))
    assert torch.equal(v, (a["beta2"] * v0) + (a["omb2"] * (gl * gl)))
    step = (a["c1"] * m.double()) / ((v.double().sqrt() * a["c2"]) + a["eps"])
    ref = theta0.double() - step
    err = (theta.double() - ref).abs()
    bound = U * theta.double().abs() + 10 * U * step.abs()
    print(f"per={per}: max |theta' - ref| / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert not torch.equal(theta, theta0)


@pytest.mark.parametrize("per", PERS)
def test_adam_three_steps_against_torch(per):
    """k = 1, 2, 3 against torch.optim.Adam in fp64 on grad = -g: max-abs <= 1e-3 lr. A condition: rounding is about
    2.4e-5 lr a step by the bound above, and the nearest wrong formula (no bias correction) is off by 2.16 lr at k = 1."""
    lr = 0.01
    theta0 = _rand(per, 5, 1.3).clamp(-4, 4)
    p = theta0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    theta, m, v = theta0, None, None
    for k in (1, 2, 3):
        w = torch.randn(6, generator=torch.Generator().manual_seed(10 * per + k)).float()
        prev = theta
        theta, m, v, g, _, _ = _step(per, w, k=k, lr=lr, theta=theta, m=m, v=v, sid=SID + k)
        p.grad = -g.double()
        opt.step()
        d = float((theta.double() - p.detach()).abs().max())
        print(f"per={per} k={k}: max |theta - Adam_fp64| = {d / lr:.2e} lr")
        assert d <= 1e-3 * lr
        if k == 1:  # the first step moves every element by +lr sign(g): ascent
            moved = (theta.double() - prev.double()) - lr * torch.sign(g.double())
            big = g.abs() > 1e-3
            assert bool(big.any()) and float(moved[big].abs().max()) <= 1e-3 * lr


# ----------------------------------------------------------------------------- 4. the engine against its parts
def _few(base):
    return GaussianDiffusionSampler(base.model, 1e-4, 0.02, T, sampler="ddim", steps=4, eta=0.0, clip_x0=True)


@pytest.fixture(scope="module")
def smp_ddpm():
    return _sampler(ARCH_TINY)


@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_engine_equals_manual_composition(smp_ddpm, kind):
    smp = _few(smp_ddpm) if kind == "ddim" else smp_ddpm
    seed, n_pairs, iters, lr = 4, 2, 2, 0.01
    n, per = 2 * n_pairs, 3 * 32 * 32
    ver = OracleVerifier()
    eng = SearchEngine(smp, ver, seed=seed)
    init = eng.initial_noise(SHAPE)
    keep = init.clone()
    best, score, h = eng.gradient_search(init, n_pairs, SIGMA, iters, lr=lr)
    assert torch.equal(init, keep), "the search modified its initial noise"
    image = eng.best_image.clone()

    theta = init.clone()
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    ws = torch.empty(rt.es_workspace_bytes(n_pairs, per), dtype=torch.uint8, device=DEV)
    b_noise, b_score, b_image, scores, norms, idx = None, float("-inf"), None, [], [], []
    for it in range(iters):
        sid = 0xB0000000 + 1 + it
        xT = rt.es_candidates(torch.empty(n, 3, 32, 32, device=DEV), theta, n, SIGMA, seed, sid)
        x = xT.clone()
        smp.run(x, seed=(seed * 1000003 + 1 + it) & MASK62, noise_offset=0)
        sc = ver.score_batch(x, n).cpu()
        bi, bs = strict_argmax(sc)
        scores.append(sc.tolist())
        idx.append(bi)
        if bs > b_score:
            b_score, b_noise, b_image = bs, xT[bi:bi + 1].clone(), x[bi:bi + 1].clone()
        if it == 0:  # candidate 3 alone: its global index keys the pair draw and the sampler's noise
            lone = rt.es_candidates(torch.empty(1, 3, 32, 32, device=DEV), theta, 1, SIGMA, seed, sid, cand_offset=3)
            assert torch.equal(lone, xT[3:4])
            smp.run(lone, seed=(seed * 1000003 + 1) & MASK62, noise_offset=3 * per)
            assert torch.equal(lone, x[3:4])
        gn2 = rt.es_step(theta, m, v, es_weights(sc, SIGMA).to(DEV), seed, sid, adam_coeffs(lr, (0.9, 0.999), 1e-8, it + 1),
                         ws)
        norms.append(gn2)
    norms = torch.cat(norms).sqrt().tolist()
    assert h["scores"] == scores and h["best_index"] == idx and h["grad_norms"] == norms
    assert score == b_score and torch.equal(best, b_noise) and torch.equal(image, b_image)
    assert h["candidates_per_iter"] == [n] * iters and eng.nfes == n * iters and len(h["pivot_rms"]) == iters
    assert h["pivot_rms"][-1] == float(theta.double().square().mean().sqrt())
    assert all(g > 0 for g in norms) and len(set(scores[0])) == n  # the scores differ: the estimate is not empty
    # the reference-API class delegates to the same search
    gs = GradientBasedSearch(iters, lr, n_pairs=n_pairs, sigma=SIGMA)
    cb, cs, ch = gs.search(init, None, ver, batched=True, sampler=smp, seed=seed)
    assert ch == h and cs == score and torch.equal(cb, best) and gs.nfes == n * iters


# ----------------------------------------------------------------------------- 5. CFG and the model verifier
def test_cfg_labels_and_model_verifier():
    smp = _sampler(TINY_CFG)
    ver = DenoisingVerifier(smp, mode="class", probes=2)
    eng = SearchEngine(smp, ver, seed=6)
    lab1 = torch.tensor([4], dtype=torch.int32, device=DEV)
    init = eng.initial_noise(SHAPE)
    best, score, h = eng.gradient_search(init, 2, SIGMA, 1, labels=lab1)
    sc = torch.tensor(h["scores"][0], dtype=torch.float64)
    assert sc.numel() == 4 and bool(torch.isfinite(sc).all()) and math.isfinite(score)
    assert h["verifier_unet_steps"] == 4 * 2  # images scored x probes
    # by hand: the labels reach the sampler and the verifier
    x = rt.es_candidates(torch.empty(4, 3, 32, 32, device=DEV), init, 4, SIGMA, 6, 0xB0000001)
    lab = lab1.repeat(4)
    smp.run(x, labels=lab, seed=(6 * 1000003 + 1) & MASK62, noise_offset=0)
    assert torch.equal(ver.score_batch(x, 4, labels=lab).cpu(), sc)
    assert torch.equal(eng.best_image, x[h["best_index"][0]][None])


# ----------------------------------------------------------------------------- 6. the entry point
def test_entry_gradient(tmp_path):
    sd = synthetic_state_dict(ARCH_TINY, 5)
    torch.save(sd, str(tmp_path / "ckpt_0_.pt"))
    out = tmp_path / "out"
    over = [f"save_weight_dir={tmp_path}", "test_load_weight=ckpt_0_.pt", "T=1000", f"inference_T={T}", "channel=32",
            "channel_mult=[1,2]", "attn=[1]", "num_res_blocks=1", "batch_size=2", "nrow=2", "seed=3",
            f"sampled_dir={out}", "search.algorithm=gradient", "search.n_pairs=2", "search.sigma=0.1",
            "search.n_iterations=2"]
    s = E.run(E.load_config(None, over))["search"]
    with open(out / "SearchBestImgs.json") as fh:
        js = json.load(fh)
    assert os.path.exists(out / "SearchBestImgs.png")
    assert js["algorithm"] == "gradient" and len(js["history"]["grad_norms"]) == 2 and js["nfes"] == 8
    assert js["history"]["grad_norms"] == s["history"]["grad_norms"] and len(js["history"]["scores"]) == 2
    # by hand: the same engine call
    net = UNet(1000, 32, [1, 2], [1], 1, 0.0).to(DEV)
    net.load_state_dict(sd)
    eng = SearchEngine(GaussianDiffusionSampler(net, 1e-4, 0.02, T), OracleVerifier(), seed=3)
    b, sc, h = eng.gradient_search(eng.initial_noise(SHAPE), 2, 0.1, 2)
    assert h == s["history"] and sc == s["best_score"] and torch.equal(b, s["best_noise"])
    assert torch.equal(eng.best_image, s["best_image"])
    with pytest.raises(ValueError, match="shaping"):
        E.run(E.load_config(None, over + ["search.shaping=softmax"]))
