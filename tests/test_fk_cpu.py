"""CPU checks of the particle search's pure parts: systematic_parents, fk_weights, resample_u, moment_scores against
the oracle's verifiers, and the entry point's ``search.algorithm: particle`` validation. No GPU, no library call.

The bound of the moment_scores check. The images are fp32 and their moments are taken here in fp64, so moment_scores'
own error is ~1e-15 relative; what differs is the oracle verifiers' fp32 arithmetic (oracle/ref_cpu.py: torch.var /
torch.std over an image's D elements, a mean over the b images, .item()). With u = 2^-24: each deviation x - mean and
its square round (3u on a term), a sum of D non-negative terms in ANY order keeps a relative error <= (D - 1) u, the
division, the square root (halving the relative error), the mean over b (b - 1 additions of non-negative terms) and the
aesthetic's final cd + ct round once more each; the mean's own error enters squared. That is within (D + 8) u
relative on a per-image variance for b <= 3, so
    oracle     |score - ref| <= (D + 8) u mean_b var     (d/dv 1/(1 + v) has magnitude <= 1)
    aesthetic  |score - ref| <= (D + 8) u |ref|
The images are 3 x 8 x 8 (D = 192): small enough that the bound (1.2e-5) separates D from D - 1 in the variance
(5e-3) and a missing shift (a factor 2)."""
import pytest
import torch

from itsd import entry as E
from itsd.search import FK_POTENTIALS, ParticleSearch, fk_weights, resample_u, systematic_parents
from itsd.verifier import AestheticPredictor, DenoisingVerifier, OracleVerifier, SelfSupervisedVerifier, moment_scores
from oracle import ref_cpu as R

U = 2.0 ** -24
US = [0.0, 0.25, 0.5, 1.0 - 2.0 ** -53, 1e-300, 0.999]


# ----------------------------------------------------------------------------- systematic_parents
@pytest.mark.parametrize("n", [1, 2, 7, 32])
@pytest.mark.parametrize("value", [1.0, 0.3, 1e-200, 7e150])
def test_uniform_weights_give_the_identity_for_every_u(n, value):
    for u in US:
        assert systematic_parents([value] * n, u) == list(range(n)), (n, value, u)


@pytest.mark.parametrize("n", [1, 5, 8])
def test_one_hot_weights_give_that_index(n):
    for k in range(n):
        w = [0.0] * n
        w[k] = 0.37
        for u in US:
            assert systematic_parents(w, u) == [k] * n


def test_counts_within_one_and_non_decreasing():
    g = torch.Generator().manual_seed(3)
    for n in (3, 8, 33):
        for trial in range(20):
            w = torch.rand(n, generator=g, dtype=torch.float64) ** 4  # (skewed)
            if trial % 3 == 0:
                w[torch.randint(0, n, (1,), generator=g)] = 0.0
            u = float(torch.rand(1, generator=g, dtype=torch.float64))
            tab = systematic_parents(w, u)
            assert len(tab) == n and all(0 <= p < n for p in tab)
            assert all(a <= b for a, b in zip(tab, tab[1:])), tab
            want = n * w / w.sum()
            for i in range(n):
                assert abs(tab.count(i) - float(want[i])) < 1.0 + 1e-9, (tab, want.tolist())
                assert w[i] > 0 or tab.count(i) == 0


def test_systematic_parents_refuses_bad_input():
    for w, u in (([], 0.5), ([0.0, 0.0], 0.5), ([1.0, -1.0], 0.5), ([1.0, float("nan")], 0.5),
                 ([1.0, float("inf")], 0.5), ([1.0, 1.0], 1.0), ([1.0, 1.0], -0.1)):
        with pytest.raises(ValueError):
            systematic_parents(w, u)


def test_resample_u_is_a_function_of_seed_and_stage():
    a, b, c = resample_u(5, 0), resample_u(5, 1), resample_u(6, 0)
    assert a == resample_u(5, 0) and 0.0 <= a < 1.0 and len({a, b, c}) == 3
    torch.manual_seed(0)
    assert resample_u(5, 0) == a  # (its own generator: not the global one)


# ----------------------------------------------------------------------------- fk_weights
def test_fk_weights_values_and_rules():
    now, prev = torch.tensor([0.5, 0.25, 1.0]), torch.tensor([0.25, 0.25, 0.0])
    w = fk_weights(now, prev, 2.0)
    assert w.dtype == torch.float64 and torch.equal(w, torch.exp(2.0 * (now.double() - prev.double())))
    assert torch.equal(fk_weights(now, 0.0, 2.0), torch.exp(2.0 * now.double()))
    assert torch.equal(fk_weights(now, prev, 0.0), torch.ones(3, dtype=torch.float64))
    nan = float("nan")
    w = fk_weights([0.5, nan, 0.1], [0.0, 0.0, nan], 1.0)
    assert w[1] == 0.0 and w[2] == 0.0 and w[0] == torch.exp(torch.tensor(0.5, dtype=torch.float64))
    assert torch.equal(fk_weights([nan, nan], [0.0, 0.0], 1.0), torch.ones(2, dtype=torch.float64))  # all zero: uniform
    assert torch.equal(fk_weights([-1e6, -2e6], [0.0, 0.0], 1.0), torch.ones(2, dtype=torch.float64))  # underflow
    assert fk_weights([1e6, 0.0, 2e6], [0.0] * 3, 1.0).tolist() == [1.0, 0.0, 1.0]  # overflow: shared
    for lam in (nan, float("inf")):
        with pytest.raises(ValueError, match="lam"):
            fk_weights([0.0], [0.0], lam)
    with pytest.raises(ValueError):
        fk_weights([0.0, 1.0], [0.0, 1.0, 2.0], 1.0)


# ----------------------------------------------------------------------------- moment_scores
def _moments(x):
    f = x.double().flatten(1)
    return torch.stack([f.sum(1), (f * f).sum(1), f.amin(1), f.amax(1)], dim=1)


@pytest.mark.parametrize("lo", [-1.0, 0.0])  # images in [-1, 1] (the aesthetic shift on) and in [0, 1] (off)
@pytest.mark.parametrize("b", [1, 3])
def test_moment_scores_against_the_oracle_verifiers(lo, b):
    n_cand, D = 4, 3 * 8 * 8
    g = torch.Generator().manual_seed(11 + b)
    x = lo + (1.0 - lo) * torch.rand(n_cand * b, 3, 8, 8, generator=g)
    assert (float(x.min()) < 0) == (lo < 0)
    m = _moments(x)
    got_o, got_a = moment_scores(m, "oracle", b, D), moment_scores(m, "aesthetic", b, D)
    assert got_o.dtype == torch.float64 and got_o.shape == (n_cand,) and got_a.shape == (n_cand,)
    for c in range(n_cand):
        img = x[c * b:(c + 1) * b]
        var64 = float(img.double().flatten(1).var(dim=1).mean())
        ro, ra = R.oracle_score(img), R.aesthetic_score(img)
        eo, ea = abs(float(got_o[c]) - ro), abs(float(got_a[c]) - ra)
        print(f"lo={lo} b={b} cand {c}: oracle err {eo:.3e} (bound {(D + 8) * U * var64:.3e}), "
              f"aesthetic err {ea:.3e} (bound {(D + 8) * U * abs(ra):.3e})")
        assert eo <= (D + 8) * U * var64
        assert ea <= (D + 8) * U * abs(ra)


def test_moment_scores_shapes_and_refusals():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(6, 3, 8, 8, generator=g) * 2 - 1
    m = _moments(x)
    rows = torch.stack([m, m.flip(0)])  # [rows, n, 4]: leading dimensions pass through
    out = moment_scores(rows, "oracle", 2, 192)
    assert out.shape == (2, 3) and torch.equal(out[0], moment_scores(m, "oracle", 2, 192))
    carried = m.clone()
    carried.per_image = 192  # (what GaussianDiffusionSampler.new_trace sets)
    assert torch.equal(moment_scores(carried, "aesthetic", 1), moment_scores(m, "aesthetic", 1, 192))
    # a candidate is shifted as a whole: one negative image halves the std of all its b images
    pos = torch.rand(2, 3, 8, 8, generator=g)
    mixed = torch.cat([pos[:1], -pos[1:]])
    assert torch.allclose(moment_scores(_moments(mixed), "aesthetic", 2, 192),
                          0.5 * moment_scores(_moments(pos), "aesthetic", 2, 192), rtol=1e-12, atol=0)
    nanrow = m.clone()
    nanrow[1] = float("nan")
    assert bool(torch.isnan(moment_scores(nanrow, "oracle", 1, 192)[1]))
    for kind in ("selfsup", "denoise", "class"):
        with pytest.raises(ValueError, match="no moment form"):
            moment_scores(m, kind, 1, 192)
    with pytest.raises(ValueError, match="per_image"):
        moment_scores(m, "oracle", 1)
    with pytest.raises(ValueError):
        moment_scores(m, "oracle", 4, 192)  # 6 images do not split into candidates of 4
    assert OracleVerifier.trace_kind == "oracle" and AestheticPredictor.trace_kind == "aesthetic"
    assert not hasattr(SelfSupervisedVerifier, "trace_kind") and not hasattr(DenoisingVerifier, "trace_kind")


# ----------------------------------------------------------------------------- config and the wrapper class
def _cfg(search=None, sampler=None):
    s = {"algorithm": "particle", "n_particles": 8, "noise_scale": 0.5, "resample_steps": [4, 2], "lam": 2.0,
         "potential": "max"}
    s.update(search or {})
    return {"search": s, "sampler": {"kind": "ddim", "steps": 6, "eta": 1.0, "clip_x0": True} if sampler is None
            else sampler}


def test_particle_config_values():
    assert E.particle_args(_cfg(), 12) == {"n_particles": 8, "noise_scale": 0.5, "resample_steps": [4, 2], "lam": 2.0,
                                           "potential": "max"}
    assert E.particle_args(_cfg({"resample_steps": 3}), 12)["resample_steps"] == [3]
    d = E.particle_args({"search": {"algorithm": "particle", "resample_steps": 1},
                         "sampler": {"kind": "ddim", "eta": 0.5}}, 12)
    assert d == {"n_particles": 4, "noise_scale": 0.1, "resample_steps": [1], "lam": 1.0, "potential": "diff"}


@pytest.mark.parametrize("key,value", [
    ("n_particles", 0), ("n_particles", 2.5), ("n_particles", True), ("noise_scale", -0.1), ("noise_scale", "x"),
    ("resample_steps", None), ("resample_steps", []), ("resample_steps", [2, 4]), ("resample_steps", [3, 3]),
    ("resample_steps", 0), ("resample_steps", 5), ("resample_steps", [4.5]), ("lam", float("nan")),
    ("lam", float("inf")), ("lam", "big"), ("potential", "sum"), ("verifier", "selfsup"), ("verifier", "denoise")])
def test_particle_config_errors_name_their_key(key, value):
    with pytest.raises(ValueError, match=rf"search\.{key}"):
        E.particle_args(_cfg({key: value}), 12)  # (6 rows: resample steps live in [1, 4])


@pytest.mark.parametrize("sampler", [{}, {"kind": "ddpm"}, {"kind": "ddim", "steps": 6},
                                     {"kind": "ddim", "steps": 6, "eta": 0.0}])
def test_particle_config_needs_a_stochastic_ddim_sampler(sampler):
    with pytest.raises(ValueError, match=r"sampler\.(kind|eta)"):
        E.particle_args(_cfg(sampler=sampler), 12)
    cfg = _cfg()
    cfg.pop("sampler")
    with pytest.raises(ValueError, match=r"sampler\.(kind|eta)"):
        E.particle_args(cfg, 12)


def test_particle_search_class():
    assert FK_POTENTIALS == ("diff", "max")
    ps = ParticleSearch(n_particles=8, resample_steps=[4, 2], noise_scale=0.5, lam=2.0, potential="max")
    assert (ps.n_particles, ps.resample_steps, ps.lam, ps.potential, ps.nfes) == (8, [4, 2], 2.0, "max", 0)
    with pytest.raises(ValueError, match="potential"):
        ParticleSearch(potential="sum")
    with pytest.raises(ValueError, match="batched"):
        ps.search(torch.zeros(1, 3, 8, 8), None, OracleVerifier())
