"""GPU tests of the branching path search: itsd_branch, the tail kernels' x0 mode (itsd_sampler_predict_x0), the
engine's stage loop against its parts, graph reuse, and the entry point. Tiny UNets with seeded synthetic weights,
T = 12, at most 8 paths.

Every tolerance is fp32 rounding of the expression under test, with eps = 2^-23 (one ulp, relative):
  itsd_branch        a*p + b*z            |d| <= 2^-23 (|a p| + |b z|)    two multiplies and one add, fused or not
  x0 vs the forward  clip(a0 x - b0 e)    |d| <= 2^-23 (|a0 x| + |b0 e|)  the same, against the forward API's own e
  x0 at t = 0        vs the sampler step  |d| <= 2^-21 (|a0 x| + |b0 e|)  two constants rounded independently
                                                                          (coeff1/2[0] vs a0/b0), plus the operations
Everything else is bit equality."""
import dataclasses
import json
import os

import pytest
import torch

from itsd import entry as E
from itsd import runtime as rt
from itsd.arch import ARCH_TINY, ARCH_TINY_CFG
from itsd.diffusion import CondGaussianDiffusionSampler, GaussianDiffusionSampler
from itsd.model import CondUNet, UNet
from itsd.schedule import renoise_coeffs, x0_coeffs
from itsd.search import PathSearch, SearchEngine, rank_desc
from itsd.verifier import OracleVerifier
from itsd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

T = 12
EPS = 2.0 ** -23
DEV = "cuda:0"
TINY_CFG = dataclasses.replace(ARCH_TINY_CFG, T=T)  # (the CFG time-embedding table has T rows)
MASK62 = (1 << 62) - 1


def _f32(v):
    """The fp32 cast of a Python float, as a Python float (what crosses the ABI)."""
    return torch.tensor(v, dtype=torch.float32).item()


def _net(a, precision="fp32", seed=0):
    if a.cfg:
        net = CondUNet(a.T, a.num_labels, a.ch, a.ch_mult, a.num_res_blocks, 0.0, img_size=a.img_size,
                       precision=precision)
    else:
        net = UNet(a.T, a.ch, a.ch_mult, a.attn, a.num_res_blocks, 0.0, img_size=a.img_size, precision=precision)
    net.load_state_dict(synthetic_state_dict(a, seed))
    return net.to(DEV)


def _sampler(a, precision="fp32"):
    net = _net(a, precision)
    if a.cfg:
        return CondGaussianDiffusionSampler(net, 1e-4, 0.028, T, w=1.8)
    return GaussianDiffusionSampler(net, 1e-4, 0.02, T)


@pytest.fixture(scope="module")
def smp_fp32():
    return _sampler(ARCH_TINY)


@pytest.fixture(scope="module")
def smp_cfg_fp32():
    return _sampler(TINY_CFG)


def _x(n, img=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, img, img, generator=g).to(DEV)


# ----------------------------------------------------------------------------- 1. itsd_branch
def _branch_case(per, n_src, parents, cand_offset, a, b, misalign=False, seed=9, sid=0xC0000001):
    n_dst = len(parents)
    g = torch.Generator().manual_seed(per)
    src = torch.randn(n_src, per, generator=g).to(DEV)
    if misalign:  # a base 4 bytes off the allocation's 16-byte alignment
        buf = torch.empty(n_dst * per + 1, device=DEV)
        dst = buf[1:].view(n_dst, per)
    else:
        dst = torch.empty(n_dst, per, device=DEV)
    dst.fill_(float("nan"))
    a32, b32 = _f32(a), _f32(b)
    rt.branch(dst, src, parents, a32, b32, seed, sid, cand_offset=cand_offset)
    z = rt.noise(torch.empty(n_dst, per, device=DEV), n_dst, seed, sid, cand_offset=cand_offset)
    p = src[torch.tensor(parents, device=DEV)].double()
    want = a32 * p + b32 * z.double()
    bound = EPS * ((a32 * p).abs() + (b32 * z.double()).abs())
    d = (dst.double() - want).abs()
    assert bool((d <= bound).all()), f"per={per} off={cand_offset}: max excess {(d - bound).max().item():.3e}"
    return dst, src, z


@pytest.mark.parametrize("per", [27, 192])  # the scalar path / the 16-byte path
@pytest.mark.parametrize("cand_offset", [7, 2 ** 31])  # 2^31: 32-bit index arithmetic would draw another z
def test_branch_vs_torch(per, cand_offset):
    _, _, z = _branch_case(per, 3, [2, 0, 0, 2, 1], cand_offset, 0.8, 0.6)
    # children of one parent differ (their draws are keyed by the child's own global index)
    assert not torch.equal(z[1], z[2])


def test_branch_copy_is_exact():
    for per in (27, 192):
        n_dst, parents = 5, [2, 0, 0, 2, 1]
        src = torch.randn(3, per, generator=torch.Generator().manual_seed(per)).to(DEV)
        dst = torch.full((n_dst, per), float("nan"), device=DEV)
        rt.branch(dst, src, parents, 1.0, 0.0, 9, 0xC0000000, cand_offset=7)
        assert torch.equal(dst, src[torch.tensor(parents, device=DEV)])


def test_branch_misaligned_base_and_many_rows():
    """per_cand % 4 == 0 on a base that is not 16-byte aligned takes the scalar path; more rows than one launch's
    parent table (256) and more than one block a row (257 16-byte items) take the chunk loop."""
    _branch_case(192, 3, [2, 0, 0, 2, 1], 7, 0.8, 0.6, misalign=True)
    parents = [(5 * j + j // 7) % 3 for j in range(300)]
    _branch_case(1028, 3, parents, 2 ** 31 - 100, 0.25, 1.5)


# ----------------------------------------------------------------------------- 2. x0 vs the forward
@pytest.mark.parametrize("t", [0, 5, T - 1])
def test_x0_vs_forward_fp32(smp_fp32, t):
    x = _x(3, seed=t)
    keep = x.clone()
    eps = smp_fp32.model(x, t).double()
    got = smp_fp32.predict_x0(x, t)
    assert torch.equal(x, keep), "predict_x0 modified x"
    a0, b0 = (_f32(v) for v in x0_coeffs(smp_fp32.sched.alphas_bar, t))
    xd = x.double()
    want = (a0 * xd - b0 * eps).clamp(-1, 1)
    bound = EPS * ((a0 * xd).abs() + (b0 * eps).abs())
    d = (got.double() - want).abs()
    assert bool((d <= bound).all()), f"t={t}: max excess {(d - bound).max().item():.3e}"
    assert got.data_ptr() != x.data_ptr()


# ----------------------------------------------------------------------------- 3. x0 at t = 0 is the last step
TAIL_CASES = {
    # id: (arch, precision, io_mfma, n)
    "tail2_f32": (ARCH_TINY, "fp32", 1, 3),
    "tail_mfma": (ARCH_TINY, "bf16", 1, 3),
    "tail2_bf16": (ARCH_TINY, "bf16", 0, 3),
    "tail_f32_cfg_128px": (dataclasses.replace(TINY_CFG, img_size=128), "fp32", 1, 2),
    "tail2_f32_cfg": (TINY_CFG, "fp32", 1, 2),
    "tail_mfma_cfg": (TINY_CFG, "bf16", 1, 2),
}


@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_x0_at_t0_is_the_samplers_last_step(case):
    """abar_0 = alpha_0, so clip(a0 x - b0 eps) and the sampler's step 0 with clip (coeff1[0] x - coeff2[0] eps, no
    noise) are the same formula: this runs the x0 epilogue of every tail kernel the launcher can select against the
    step epilogue of the same kernel.
      tail2_f32           fp32, 32 px                      -> tail2_kernel<float>
      tail_mfma           bf16, 32 px                      -> tail_mfma_kernel
      tail2_bf16          bf16, 32 px, "io_mfma" 0         -> tail2_kernel<bf16_t> (the option is read at create)
      tail_f32_cfg_128px  fp32 CFG, 128 px (128 does not divide 64), n = 2, w = 1.8
                                                           -> tail_kernel<float>, guided eps on the doubled batch
      tail2_f32_cfg       fp32 CFG, 32 px, n = 2, w = 1.8  -> tail2_kernel<float>, guided
      tail_mfma_cfg       bf16 CFG, 32 px, n = 2, w = 1.8  -> tail_mfma_kernel, guided (two passes)"""
    a, precision, io_mfma, n = TAIL_CASES[case]
    rt.set_option("io_mfma", io_mfma)
    try:
        smp = _sampler(a, precision)
        x = _x(n, a.img_size, seed=3)
        lab = torch.tensor([3, 7], dtype=torch.int32, device=DEV)[:n] if a.cfg else None
        keep = x.clone()
        got = smp.predict_x0(x, 0, labels=lab)  # (creates the native handle: inside the option window)
        assert torch.equal(x, keep)
        step = smp.run(x.clone(), t_begin=0, t_end=0, labels=lab, seed=1, clip=True)
        if a.cfg:
            eps = (1.0 + smp.w) * smp.model(x, 0, lab).double() - smp.w * smp.model(x, 0, torch.zeros_like(lab)).double()
        else:
            eps = smp.model(x, 0).double()
    finally:
        rt.set_option("io_mfma", 1)
    a0, b0 = (_f32(v) for v in x0_coeffs(smp.sched.alphas_bar, 0))
    bound = 4 * EPS * ((a0 * x.double()).abs() + (b0 * eps).abs())  # 2^-21
    d = (got.double() - step.double()).abs()
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0
    assert bool((d <= bound).all()), f"{case}: max excess {(d - bound).max().item():.3e}"


# ----------------------------------------------------------------------------- 4. the placeholder is untouched
def test_placeholder_unchanged_by_a_branching_search(smp_fp32):
    eng = SearchEngine(smp_fp32, OracleVerifier(), seed=4)
    init = eng.initial_noise((1, 3, 32, 32))
    b0, s0, h0 = eng.path_search(init, 4, 0.1, 400)
    img0 = eng.best_image.clone()
    eng.path_search_branch(init, 4, 0.1, [8, 3], keep=2, renoise_steps=2)
    b1, s1, h1 = eng.path_search(init, 4, 0.1, 400)
    assert h0 == h1 and s0 == s1 and torch.equal(b0, b1) and torch.equal(img0, eng.best_image)
    assert set(h1) == {"scores", "injection_points", "best_index"} and h1["injection_points"] == [400] * 4


def test_noop_stage_equals_the_placeholder_round(smp_fp32, monkeypatch):
    """One stage that changes nothing (keep = N, descending stage scores: parents = identity; renoise_steps = 0:
    a = 1, b = 0) is the placeholder round run as two windows: pins the window split, the key of window 0 (and that
    it is kept while no step is re-run), and that the a = 1, b = 0 branch is an exact copy."""
    ver = OracleVerifier()
    eng = SearchEngine(smp_fp32, ver, seed=4)
    init = eng.initial_noise((1, 3, 32, 32))
    rb, rs, rh = eng.path_search(init, 4, 0.1, 400)
    rimg = eng.best_image.clone()
    real, calls = ver.score_batch, []

    def fake(images, n_cand):
        calls.append(n_cand)
        if len(calls) == 1:  # the stage's scores
            return torch.arange(n_cand, 0, -1, dtype=torch.float64, device=images.device)
        return real(images, n_cand)

    monkeypatch.setattr(ver, "score_batch", fake)
    b, s, h = eng.path_search_branch(init, 4, 0.1, [5], keep=4, renoise_steps=0)
    assert h["parents"] == [[0, 1, 2, 3]] and len(calls) == 2
    assert h["scores"] == rh["scores"] and h["best_index"] == rh["best_index"] == h["root_index"] and s == rs
    assert torch.equal(b, rb) and torch.equal(eng.best_image, rimg)


# ----------------------------------------------------------------------------- 5. the engine equals its parts
def _by_hand(smp, ver, seed, init, n, scale, steps, keep, delta, labels=None, graph=True):
    """The search from its documented parts: candidates of round 0; window 0 under the placeholder's key
    seed * 1000003, window i >= 1 under seed * 1000003 + 0x5B000000 + i when renoise_steps > 0 (else the same key);
    branch draws from Philox stream 0xC0000000 + stage, keyed by the child's global index."""
    shape = tuple(init.shape)
    eng = SearchEngine(smp, ver, seed=seed)
    x = eng.candidate_noise(0, 0, n, shape, init, scale)
    lab = None if labels is None else labels.flatten().repeat(n)
    key = lambda i: (seed * 1000003 + (0x5B000000 + i if (i and delta) else 0)) & MASK62
    t_hi, stage_scores, parents = T - 1, [], []
    for i, s in enumerate(steps):
        if t_hi > s:
            smp.run(x, t_begin=t_hi, t_end=s + 1, labels=lab, seed=key(i), noise_offset=0, graph=graph, clip=False)
        sc = ver.score_batch(smp.predict_x0(x, s, labels=lab), n).cpu()
        order, m = rank_desc(sc), n // keep
        tab = [order[j // m] for j in range(n)]
        a, b = renoise_coeffs(smp.sched.alphas_bar, s, delta)
        x = rt.branch(torch.empty_like(x), x, tab, a, b, seed, 0xC0000000 + i, cand_offset=0)
        stage_scores.append(sc.tolist())
        parents.append(tab)
        t_hi = s + delta
    smp.run(x, t_begin=t_hi, t_end=0, labels=lab, seed=key(len(steps)), noise_offset=0, graph=graph, clip=True)
    return x, ver.score_batch(x, n).cpu(), stage_scores, parents


def _check_engine(smp, n, steps, keep, delta, labels=None):
    ver, seed = OracleVerifier(), 6
    eng = SearchEngine(smp, ver, seed=seed)
    init = eng.initial_noise((1, 3, 32, 32))
    best, score, h = eng.path_search_branch(init, n, 0.5, steps, keep=keep, renoise_steps=delta, labels=labels)
    x, sc, stage_scores, parents = _by_hand(smp, ver, seed, init, n, 0.5, steps, keep, delta, labels)
    assert h["stage_scores"] == stage_scores and h["parents"] == parents and h["scores"] == sc.tolist()
    bi = int(torch.argmax(torch.nan_to_num(sc, nan=float("-inf"))))
    root = bi
    for tab in reversed(parents):
        root = tab[root]
    assert h["best_index"] == bi and h["root_index"] == root and score == float(sc[bi])
    assert torch.equal(eng.best_image, x[bi:bi + 1])
    assert torch.equal(best, eng.candidate_noise(0, root, 1, (1, 3, 32, 32), init, 0.5))
    assert h["injection_points"] == list(steps) and eng.nfes == n
    return h


def test_engine_equals_its_parts_fp32(smp_fp32):
    h = _check_engine(smp_fp32, 8, [8, 3], 2, 2)
    assert h["unet_steps"] == 8 * ((3 + 7 + 6) + 2)


def test_engine_equals_its_parts_cfg(smp_cfg_fp32):
    lab = torch.tensor([4], dtype=torch.int32, device=DEV)
    h = _check_engine(smp_cfg_fp32, 4, [6], 2, 2, labels=lab)
    assert h["unet_steps"] == 4 * ((5 + 9) + 1)


def test_product_class_branch_mode(smp_fp32):
    """PathSearch(mode="branch").search(batched=True) is the engine's search (int or list injection_step)."""
    init = SearchEngine(smp_fp32, OracleVerifier(), seed=2).initial_noise((1, 3, 32, 32))
    ps = PathSearch(n_paths=4, injection_step=[8, 3], noise_scale=0.5, mode="branch", keep=2, renoise_steps=1)
    b, s, h = ps.search(init, None, OracleVerifier(), batched=True, sampler=smp_fp32, seed=2)
    eb, es, eh = SearchEngine(smp_fp32, OracleVerifier(), seed=2).path_search_branch(init, 4, 0.5, [8, 3], 2, 1)
    assert h == eh and s == es and torch.equal(b, eb) and ps.nfes == 4
    ps1 = PathSearch(n_paths=4, injection_step=5, noise_scale=0.5, mode="branch")  # keep defaults to 1
    _, _, h1 = ps1.search(init, None, OracleVerifier(), batched=True, sampler=smp_fp32, seed=2)
    assert h1["injection_points"] == [5] and len(set(h1["parents"][0])) == 1


# ----------------------------------------------------------------------------- 6. graph reuse
def test_one_step_graph_serves_every_window():
    smp = _sampler(ARCH_TINY)  # its own handle: the capture count starts at 0
    res = {}
    for graph in (True, False):
        eng = SearchEngine(smp, OracleVerifier(), seed=8, graph=graph)
        init = eng.initial_noise((1, 3, 32, 32))
        eng.reserve(8, (1, 3, 32, 32))
        before = smp._native(8).query("graph_captures")
        _, s, h = eng.path_search_branch(init, 8, 0.5, [8, 3], keep=2, renoise_steps=2)
        grown = smp._native(8).query("graph_captures") - before
        assert grown <= (1 if graph else 0), f"graph={graph}: {grown} captures"  # all windows share n; x0 runs eagerly
        res[graph] = (s, h, eng.best_image.clone())
    assert res[True][0] == res[False][0] and res[True][1] == res[False][1]
    assert torch.equal(res[True][2], res[False][2])


# ----------------------------------------------------------------------------- 7. the entry point
def test_entry_path_mode_branch(tmp_path):
    a = ARCH_TINY
    sd = synthetic_state_dict(a, 5)
    torch.save(sd, str(tmp_path / "ckpt_0_.pt"))
    base = [f"save_weight_dir={tmp_path}", "test_load_weight=ckpt_0_.pt", "T=1000", f"inference_T={T}", "channel=32",
            "channel_mult=[1,2]", "attn=[1]", "num_res_blocks=1", "batch_size=2", "nrow=2", "seed=3",
            "search.algorithm=path", "search.n_paths=8", "search.injection_step=[8,3]", "search.noise_scale=0.5"]
    out_b, out_p = tmp_path / "branch", tmp_path / "plain"
    res = E.run(E.load_config(None, base + [f"sampled_dir={out_b}", "search.path_mode=branch", "search.renoise_steps=2"]))
    s = res["search"]
    with open(out_b / "SearchBestImgs.json") as fh:
        js = json.load(fh)
    assert os.path.exists(out_b / "SearchBestImgs.png")
    assert js["history"]["injection_points"] == [8, 3] and js["history"]["parents"] == s["history"]["parents"]
    assert len(js["history"]["parents"]) == 2 and all(len(p) == 8 for p in js["history"]["parents"])
    assert len(set(js["history"]["parents"][0])) == 2  # keep defaults to max(1, 8 // 4) = 2
    assert js["nfes"] == 8 and s["best_image"].shape == (1, 3, 32, 32)
    # by hand: the same engine call
    net = UNet(1000, 32, [1, 2], [1], 1, 0.0).to(DEV)
    net.load_state_dict(sd)
    smp = GaussianDiffusionSampler(net, 1e-4, 0.02, T)
    eng = SearchEngine(smp, OracleVerifier(), seed=3)
    init = eng.initial_noise((1, 3, 32, 32))
    _, hs, hh = eng.path_search_branch(init, 8, 0.5, [8, 3], keep=2, renoise_steps=2)
    assert hh == s["history"] and hs == s["best_score"] and torch.equal(eng.best_image, s["best_image"])
    # without path_mode: the placeholder, as before
    res = E.run(E.load_config(None, base + [f"sampled_dir={out_p}"]))
    p = res["search"]
    pb, pscore, ph = eng.path_search(init, 8, 0.5, 8)
    assert p["history"] == ph and p["best_score"] == pscore and torch.equal(p["best_noise"], pb)
    assert "parents" not in p["history"] and p["history"]["injection_points"] == [8] * 8
