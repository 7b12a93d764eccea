"""The gradient search without autograd (GradientBasedSearch / SearchEngine.gradient_search) on the CPU: the pair
weights of the antithetic ES estimate, Adam's host constants, the refusals, an ascent test through the sequential class
and through the engine loop on stand-ins, and the world-size-2 gloo protocol (one collective an iteration) against the
single-process run. The engine's three device hooks -- es_candidates, es_workspace, es_update -- are overridden with
plain-torch restatements of what the kernels compute; the kernels themselves are covered by tests/test_gpu_es_search.py."""
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from itsd import runtime as rt
from itsd import search as S
from itsd.schedule import adam_coeffs
from itsd.search import GradientBasedSearch, SearchEngine, es_weights, strict_argmax

NAN = float("nan")
SHAPE = (1, 3, 8, 8)


def _hash_field(shape):
    """A fixed field in [-1, 1)."""
    i = torch.arange(torch.Size(shape).numel(), dtype=torch.float64)
    v = torch.sin(i * 12.9898 + 4.1) * 43758.5453
    return ((v - torch.floor(v)) * 2 - 1).float().view(shape)


TARGET = _hash_field(SHAPE)


def _f(x):
    return -((x.double() - TARGET.double()) ** 2).mean().item()


F0 = _f(torch.zeros(SHAPE))


# ----------------------------------------------------------------------------- es_weights
def test_es_weights_raw_scale_and_sign():
    w = es_weights([1.0, 0.0, 0.0, 2.0], sigma=0.5)  # M = 2: 1 / (2 M sigma) = 0.5
    assert w.dtype == torch.float32 and w.tolist() == [0.5, -1.0]
    w = es_weights(torch.tensor([3.0, 1.0], dtype=torch.float64), sigma=0.25)  # M = 1: 1 / 0.5
    assert w.tolist() == [4.0]
    # fp64 inside: a difference fp32 scores would lose
    w = es_weights(torch.tensor([1.0 + 2.0 ** -40, 1.0], dtype=torch.float64), sigma=0.5)
    assert w.tolist() == [2.0 ** -40]


def test_es_weights_nan_pair_is_zero():
    w = es_weights([NAN, 1.0, 2.0, NAN, float("inf"), 0.0, float("inf"), float("inf"), 5.0, 1.0], sigma=0.1)
    assert w[:4].tolist() == [0.0, 0.0, 0.0, 0.0]  # NaN, NaN, inf, inf - inf
    assert w[4].item() == pytest.approx(4.0 / (10 * 0.1))


def test_es_weights_ties():
    assert es_weights([2.0, 2.0, 1.0, 1.0], sigma=0.1).tolist() == [0.0, 0.0]
    # rank shaping breaks a tie towards the lower index: places 0, 1 -> u = 1/2, 1/6; places 2, 3 -> -1/6, -1/2
    w = es_weights([2.0, 2.0, 1.0, 1.0], sigma=0.25, shaping="rank")
    assert torch.allclose(w.double(), torch.tensor([1 / 3, 1 / 3], dtype=torch.float64), atol=1e-7)


def test_es_weights_rank_utilities_n4():
    # scores 0.1 (place 2), 0.9 (place 0), NaN (place 3: last), 0.5 (place 1); u = 0.5 - place / 3
    u = [0.5 - 2 / 3, 0.5, 0.5 - 1.0, 0.5 - 1 / 3]
    w = es_weights([0.1, 0.9, NAN, 0.5], sigma=0.5, shaping="rank")
    want = torch.tensor([(u[0] - u[1]) / 2.0, (u[2] - u[3]) / 2.0], dtype=torch.float64)
    assert torch.allclose(w.double(), want, atol=1e-7)
    # utilities are centred (they sum to zero) and depend on the order alone
    assert torch.equal(w, es_weights([-7.0, 1e6, NAN, 3.0], sigma=0.5, shaping="rank"))


def test_es_weights_refusals():
    for bad in (dict(scores=[1.0, 2.0], sigma=0.1, shaping="softmax"), dict(scores=[1.0, 2.0], sigma=0.0),
                dict(scores=[1.0, 2.0, 3.0], sigma=0.1), dict(scores=[], sigma=0.1)):
        with pytest.raises(ValueError):
            es_weights(**bad)


# ----------------------------------------------------------------------------- adam_coeffs
@pytest.mark.parametrize("k", [1, 2, 10])
def test_adam_coeffs_closed_forms(k):
    lr, b1, b2, eps = 0.01, 0.9, 0.999, 1e-8
    c = adam_coeffs(lr, (b1, b2), eps, k)
    assert c is not None and rt.adam_coeffs is adam_coeffs
    assert c["beta1"] == b1 and c["beta2"] == b2 and c["eps"] == eps
    assert c["omb1"] == 1.0 - b1 and c["omb2"] == 1.0 - b2
    # 1 - beta^k = (1 - beta)(1 + beta + ... + beta^(k-1))
    g1 = (1.0 - b1) * sum(b1 ** i for i in range(k))
    g2 = (1.0 - b2) * sum(b2 ** i for i in range(k))
    assert c["c1"] == pytest.approx(lr / g1, rel=1e-12)
    assert c["c2"] == pytest.approx(1.0 / math.sqrt(g2), rel=1e-12)
    if k == 1:  # the first step of Adam moves by lr: c1 omb1 = lr, c2^2 omb2 = 1
        assert c["c1"] * c["omb1"] == pytest.approx(lr, rel=1e-12)
        assert c["c2"] ** 2 * c["omb2"] == pytest.approx(1.0, rel=1e-12)


def test_adam_coeffs_refusals():
    for bad in ((0.01, (1.0, 0.999), 1e-8, 1), (0.01, (0.9, -0.1), 1e-8, 1), (0.01, (0.9, 0.999), 0.0, 1),
                (0.0, (0.9, 0.999), 1e-8, 1), (0.01, (0.9, 0.999), 1e-8, 0)):
        with pytest.raises(ValueError):
            adam_coeffs(*bad)


# ----------------------------------------------------------------------------- stand-ins
class _Model:
    device = torch.device("cpu")


class _Sampler:
    """The identity sampler: the score is a deterministic function of x_T."""
    model = _Model()
    T = 4

    def __init__(self):
        self.runs = []

    def run(self, x, labels=None, seed=0, noise_offset=0, graph=True):
        self.runs.append((seed, noise_offset, x.shape[0]))
        return x


class _Verifier:
    kind = 0

    def score_batch(self, images, n_cand):
        d = images.reshape(n_cand, -1).double() - TARGET.reshape(1, -1).double()
        return -(d ** 2).mean(dim=1)


class CPUEngine(SearchEngine):
    """The device hooks in plain torch: z_p a pure function of (seed, round, pair); the update the stated fp32
    expressions (include/itsd.h, itsd_es_step) with a one-level sum."""
    sign = 1.0  # -1.0: the estimate's sign flipped (what the ascent condition must tell apart)

    def _z(self, round_id, p, shape):
        gen = torch.Generator().manual_seed(self.seed * 1_000_003 + round_id * 10_007 + p)
        return torch.randn(shape, generator=gen)

    def es_candidates(self, round_id, g0, count, shape, pivot, sigma):
        return torch.cat([pivot + ((-sigma if c & 1 else sigma) * self._z(round_id, c >> 1, shape))
                          for c in range(g0, g0 + count)])

    def es_workspace(self, n_pairs, per):
        return None

    def es_update(self, round_id, theta, m, v, w, adam, ws, gnorm2):
        g = torch.zeros_like(theta)
        for p in range(w.numel()):
            g += w[p] * self._z(round_id, p, tuple(theta.shape))
        a = {k: torch.tensor(x, dtype=torch.float32) for k, x in adam.items()}
        gl = -(self.sign * g)
        m.copy_(a["beta1"] * m + a["omb1"] * gl)
        v.copy_(a["beta2"] * v + a["omb2"] * (gl * gl))
        theta.sub_((a["c1"] * m) / (v.sqrt() * a["c2"] + a["eps"]))
        gnorm2.copy_(g.double().square().sum().reshape(1))


def _engine_search(eng, shaping="raw", n_iterations=60, **kw):
    args = dict(n_pairs=8, sigma=0.1, n_iterations=n_iterations, lr=0.05, shaping=shaping)
    args.update(kw)
    return eng.gradient_search(torch.zeros(SHAPE), **args)


# ----------------------------------------------------------------------------- ascent
@pytest.mark.parametrize("shaping", ["raw", "rank"])
@pytest.mark.parametrize("seed", range(5))
def test_sequential_class_ascends(shaping, seed):
    """f(x) = -mean((x - t)^2) from theta_0 = 0: 60 Adam steps on the ES estimate must at least halve |f|. (A
    plain-torch restatement reads 0.14-0.26 of f(theta_0); with the gradient's sign flipped it stays at 0.98-1.0.)"""
    torch.manual_seed(seed)
    gs = GradientBasedSearch(60, 0.05, n_pairs=8, sigma=0.1, shaping=shaping)
    calls = []

    def denoise(x, **kw):
        calls.append(torch.is_grad_enabled())
        return x

    best, score, hist = gs.search(torch.zeros(SHAPE), denoise, lambda x, **kw: _f(x), device="cpu")
    assert score > F0 / 2, (score, F0)
    assert _f(best) == score                      # best_noise is the candidate that earned best_score
    assert gs.nfes == 60 * 16 and len(calls) == 60 * 16 and not any(calls)  # under no_grad
    assert set(hist) == {"scores", "grad_norms"}  # the reference's keys
    assert len(hist["scores"]) == 60 and all(len(s) == 16 for s in hist["scores"])
    assert len(hist["grad_norms"]) == 60 and all(g > 0 for g in hist["grad_norms"])
    assert score == max(max(s) for s in hist["scores"])
    gs.reset_nfes()
    assert gs.nfes == 0


@pytest.mark.parametrize("shaping", ["raw", "rank"])
@pytest.mark.parametrize("seed", range(5))
def test_engine_loop_ascends(shaping, seed):
    eng = CPUEngine(_Sampler(), _Verifier(), seed=seed)
    best, score, hist = _engine_search(eng, shaping)
    assert score > F0 / 2, (score, F0)
    assert _f(best) == pytest.approx(score, abs=1e-12)
    assert _f(eng.best_image) == pytest.approx(score, abs=1e-12)  # the identity sampler: the image is the noise


def test_flipped_sign_does_not_ascend():
    """The condition separates ascent from descent: the same loop with -g never gets near f(theta_0) / 2."""
    class Flipped(CPUEngine):
        sign = -1.0

    _, score, _ = _engine_search(Flipped(_Sampler(), _Verifier(), seed=0))
    assert score < 0.9 * F0  # (scores are negative: this is within 10 % of where it started)


# ----------------------------------------------------------------------------- the loop's bookkeeping
def test_engine_bookkeeping_and_keys():
    smp = _Sampler()
    eng = CPUEngine(smp, _Verifier(), seed=3)
    best, score, h = _engine_search(eng, n_iterations=3, n_pairs=2)
    assert set(h) == {"scores", "grad_norms", "best_index", "candidates_per_iter", "pivot_rms"}
    assert h["candidates_per_iter"] == [4, 4, 4] and eng.nfes == 12
    assert len(h["grad_norms"]) == 3 and len(h["pivot_rms"]) == 3 and all(len(s) == 4 for s in h["scores"])
    for sc, bi in zip(h["scores"], h["best_index"]):
        assert bi == strict_argmax(torch.tensor(sc, dtype=torch.float64))[0]
    assert score == max(max(s) for s in h["scores"])
    # the sampler keys of run_round: round id 1 + it, noise offset of the shard's first candidate
    assert smp.runs == [((3 * 1000003 + 1 + it) & ((1 << 62) - 1), 0, 4) for it in range(3)]
    # at k = 1 Adam moves every element by lr: sqrt(mean theta^2) = lr exactly where g != 0
    assert h["pivot_rms"][0] == pytest.approx(0.05, rel=1e-4)
    # best_noise: regenerated from the PRE-update pivot of the iteration that found it, so it scores best_score
    assert _f(best) == pytest.approx(score, abs=1e-12)
    assert S._STREAM_ES == 0xB0000000


def test_all_nan_scores_keep_the_initial_noise():
    class NaNVerifier(_Verifier):
        def score_batch(self, images, n_cand):
            return torch.full((n_cand,), NAN, dtype=torch.float64)

    eng = CPUEngine(_Sampler(), NaNVerifier(), seed=0)
    init = torch.ones(SHAPE)
    best, score, h = eng.gradient_search(init, 2, 0.1, 2)
    assert torch.equal(best, init) and score == float("-inf") and h["best_index"] == [-1, -1]
    assert h["grad_norms"] == [0.0, 0.0] and eng.best_image is None  # a NaN score never steers
    assert h["pivot_rms"] == [1.0, 1.0]


def test_labels_are_repeated_and_model_verifier_steps_counted():
    class Ctx(_Verifier):
        needs_context, probes = True, 3
        seen = []

        def score_batch(self, images, n_cand, labels=None):
            self.seen.append(labels.tolist())
            return super().score_batch(images, n_cand)

    eng = CPUEngine(_Sampler(), Ctx(), seed=0)
    _, _, h = eng.gradient_search(torch.zeros(SHAPE), 2, 0.1, 2, labels=torch.tensor([7]))
    assert Ctx.seen == [[7, 7, 7, 7]] * 2
    assert h["verifier_unet_steps"] == 2 * 4 * 3  # images scored x probes


@pytest.mark.parametrize("kw", [dict(n_pairs=0), dict(n_pairs=-2), dict(sigma=0.0), dict(sigma=-0.1),
                                dict(sigma=float("nan")), dict(shaping="softmax"), dict(lr=0.0),
                                dict(betas=(1.0, 0.999))])
def test_refusals(kw):
    smp = _Sampler()
    eng = CPUEngine(smp, _Verifier(), seed=0)
    with pytest.raises(ValueError):
        _engine_search(eng, **kw)
    assert smp.runs == [] and eng.nfes == 0  # refused before any work


def test_reference_noise_is_refused():
    eng = CPUEngine(_Sampler(), _Verifier(), seed=0, noise="reference")
    with pytest.raises(ValueError, match="reference"):
        _engine_search(eng)


def test_class_constructor_and_batched_delegation():
    g = GradientBasedSearch()
    assert (g.n_iterations, g.lr, g.verbose, g.n_pairs, g.sigma, g.shaping) == (20, 0.01, False, 4, 0.05, "raw")
    assert (g.betas, g.eps, g.nfes) == ((0.9, 0.999), 1e-8, 0)
    g = GradientBasedSearch(5, 0.1, True)  # the reference's positional constructor
    assert (g.n_iterations, g.lr, g.verbose) == (5, 0.1, True)
    with pytest.raises(TypeError):
        GradientBasedSearch(5, 0.1, True, 8)  # the new parameters are keyword-only
    for bad in (dict(shaping="softmax"), dict(n_pairs=0), dict(sigma=0.0)):
        with pytest.raises(ValueError):
            GradientBasedSearch(**bad)
    with pytest.raises(ValueError, match="sampler"):
        GradientBasedSearch().search(torch.zeros(SHAPE), None, _Verifier(), batched=True)


# ----------------------------------------------------------------------------- sharded
def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    count = {"all_gather": 0, "broadcast": 0}
    for name in count:
        def wrapped(*a, _f=getattr(dist, name), _n=name, **k):
            count[_n] += 1
            return _f(*a, **k)
        setattr(dist, name, wrapped)
    eng = CPUEngine(_Sampler(), _Verifier(), seed=3)
    best, score, h = _engine_search(eng, n_iterations=4, n_pairs=3)
    torch.save({"best": best, "score": score, "hist": h, "image": eng.best_image.clone(), "count": count,
                "runs": eng.sampler.runs}, f"{out_path}.{rank}")
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world2_equals_single_process():
    """N = 6 over two ranks: rank 1's shard starts on a minus candidate (global index 3)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "res")
        mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
        rs = [torch.load(f"{out}.{r}", weights_only=False) for r in (0, 1)]
    single = CPUEngine(_Sampler(), _Verifier(), seed=3)
    best, score, h = _engine_search(single, n_iterations=4, n_pairs=3)
    for rank, r in enumerate(rs):
        assert r["hist"]["scores"] == h["scores"] and r["hist"]["best_index"] == h["best_index"]
        assert r["hist"]["grad_norms"] == h["grad_norms"] and r["hist"]["pivot_rms"] == h["pivot_rms"]
        assert r["score"] == score and torch.equal(r["best"], best) and torch.equal(r["image"], single.best_image)
        assert r["count"] == {"all_gather": 4, "broadcast": 1}  # one collective an iteration + the final broadcast
        assert [x[1:] for x in r["runs"]] == [(rank * 3 * 192, 3)] * 4  # keyed by the shard's global position


def test_candidates_must_split_over_the_ranks():
    eng = CPUEngine(_Sampler(), _Verifier(), seed=0)
    eng.world = 4  # (as under a 4-rank group)
    with pytest.raises(ValueError, match="split"):
        _engine_search(eng, n_pairs=3)  # N = 6 over 4 ranks
