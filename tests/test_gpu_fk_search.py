"""GPU tests of the particle search (SearchEngine.fk_search) on the sampler's score trace. ARCH_TINY with seeded
synthetic weights, fp32, T = 12 under ddim with 6 rows, eta = 1; 8 particles. The weights are synthetic: nothing here
says resampling finds better images, the checks pin mechanics. Everything is bit equality."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from itsd import entry as E
from itsd import runtime as rt
from itsd.arch import ARCH_TINY
from itsd.diffusion import GaussianDiffusionSampler
from itsd.model import UNet
from itsd.search import (ParticleSearch, SearchEngine, fk_weights, resample_u, root_of, strict_argmax,
                         systematic_parents)
from itsd.verifier import AestheticPredictor, OracleVerifier, SelfSupervisedVerifier, moment_scores
from itsd.weights import synthetic_state_dict
from test_gpu_path_branch import DEV, MASK62, T, _sampler
from test_gpu_x0_trace import K, _ddim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (1, 3, 32, 32)
D = 3 * 32 * 32
N = 8


@pytest.fixture(scope="module")
def smp():
    return _ddim(ARCH_TINY)


def _by_hand(smp, ver, seed, init, n, scale, steps, lam, potential):
    """The search from its documented parts: round 0's candidates; every window traced under the placeholder's key
    seed * 1000003; a stage's scores = moment_scores of trace row s + 1; fk_weights of the potential;
    systematic_parents with resample_u(seed, stage); exact copies by rt.branch with (1, 0)."""
    eng = SearchEngine(smp, ver, seed=seed)
    x = eng.candidate_noise(0, 0, n, SHAPE, init, scale)
    key = (seed * 1000003) & MASK62
    trace = smp.new_trace(n)
    prev = torch.zeros(n, dtype=torch.float64)
    run_max, prev_max = torch.full((n,), float("-inf"), dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    t_hi, out = K - 1, {"stage_scores": [], "weights": [], "ess": [], "parents": [], "trace_scores": []}
    for i, s in enumerate(steps):
        smp.run(x, t_begin=t_hi, t_end=s + 1, seed=key, noise_offset=0, clip=False, trace=trace)
        win = torch.stack([moment_scores(trace[k], ver.trace_kind, 1, D) for k in range(t_hi, s, -1)]).cpu()
        now = win[-1]
        if potential == "diff":
            w = fk_weights(now, prev, lam)
        else:
            run_max = torch.maximum(run_max, win.amax(dim=0))
            w = fk_weights(run_max, prev_max, lam)
        tab = systematic_parents(w, resample_u(seed, i))
        x = rt.branch(torch.empty_like(x), x, tab, 1.0, 0.0, seed, 0xC0000000 + i, cand_offset=0)
        idx = torch.tensor(tab)
        prev, run_max = now[idx], run_max[idx]
        prev_max = run_max.clone()
        out["stage_scores"].append(now.tolist())
        out["weights"].append(w.tolist())
        out["ess"].append(float(w.sum() ** 2 / (w * w).sum()))
        out["parents"].append(tab)
        out["trace_scores"] += win.tolist()
        t_hi = s
    smp.run(x, t_begin=t_hi, t_end=0, seed=key, noise_offset=0, clip=True, trace=trace)
    out["trace_scores"] += [moment_scores(trace[k], ver.trace_kind, 1, D).tolist() for k in range(t_hi, -1, -1)]
    return x, ver.score_batch(x, n).cpu(), out


@pytest.mark.parametrize("potential,ver", [("diff", OracleVerifier()), ("max", AestheticPredictor())],
                         ids=["diff-oracle", "max-aesthetic"])
def test_engine_equals_its_parts(smp, potential, ver):
    seed, steps, lam, scale = 6, [4, 2], 300.0, 0.5
    eng = SearchEngine(smp, ver, seed=seed)
    init = eng.initial_noise(SHAPE)
    best, score, h = eng.fk_search(init, N, scale, steps, lam, potential=potential)
    x, sc, want = _by_hand(smp, ver, seed, init, N, scale, steps, lam, potential)
    print(f"{potential}: parents {h['parents']} ess {h['ess']}")
    for k in ("stage_scores", "weights", "parents", "trace_scores"):
        assert h[k] == want[k], k
    # (two fp64 formulas of one number, (sum w)^2 / sum w^2 and 1 / sum w~^2: a few fp64 roundings of N = 8 terms)
    assert all(abs(a - b) <= 1e-12 * b for a, b in zip(h["ess"], want["ess"])) and all(1.0 <= e <= N for e in h["ess"])
    assert h["scores"] == sc.tolist()
    assert any(tab != list(range(N)) for tab in h["parents"]), "no stage resampled: the case shows nothing"
    bi, bs = strict_argmax(sc)
    root = root_of(h["parents"], bi)
    assert h["best_index"] == bi and h["root_index"] == root and score == bs
    assert torch.equal(eng.best_image, x[bi:bi + 1])
    assert torch.equal(best, eng.candidate_noise(0, root, 1, SHAPE, init, scale))
    assert h["unet_steps"] == N * K and eng.nfes == N  # no per-stage term: a stage costs no evaluation
    assert len(h["trace_scores"]) == K and all(len(r) == N for r in h["trace_scores"])
    assert h["resample_steps"] == steps and h["potential"] == potential


def test_lam_zero_is_the_plain_round(smp):
    """lam = 0: every weight is 1, every table the identity, every copy exact, the window key unchanged: the search
    is path_search's round bit for bit."""
    eng = SearchEngine(smp, OracleVerifier(), seed=4)
    init = eng.initial_noise(SHAPE)
    pb, pscore, ph = eng.path_search(init, N, 0.5, 400)
    pimg = eng.best_image.clone()
    for potential in ("diff", "max"):
        b, s, h = eng.fk_search(init, N, 0.5, [4, 3, 1], 0.0, potential=potential)
        assert h["parents"] == [list(range(N))] * 3 and h["ess"] == [float(N)] * 3
        assert h["scores"] == ph["scores"] and h["best_index"] == ph["best_index"] == h["root_index"] and s == pscore
        assert torch.equal(b, pb) and torch.equal(eng.best_image, pimg)


class _Spiked:
    """A sampler stand-in: the real sampler, except that after a traced window that ran `row` the trace entry of
    particle `col` at that row is overwritten with the moments of a constant image (variance 0: the oracle score
    1.0, above every real score)."""

    def __init__(self, smp, row, col):
        self._smp, self.row, self.col = smp, row, col

    def __getattr__(self, k):
        return getattr(self._smp, k)

    def run(self, x, **kw):
        out = self._smp.run(x, **kw)
        if kw.get("trace") is not None and kw["t_end"] <= self.row <= kw["t_begin"]:
            kw["trace"][self.row, self.col] = 0.0
        return out


def test_max_potential_reads_every_row(smp):
    """Which of the two ways: the test overwrites a mid-window trace row through a sampler stand-in. One stage at
    row 2: its window runs rows 5, 4, 3 and the stage score is row 3's. Row 4 of particle 5 is spiked to the score
    1.0. `max` sees it (the running maximum covers every row run) and every child descends from particle 5; `diff`
    reads row 3 only and is the search on the real sampler."""
    seed, lam, col = 9, 500.0, 5
    init = SearchEngine(smp, OracleVerifier(), seed=seed).initial_noise(SHAPE)
    res = {}
    for potential in ("diff", "max"):
        for spiked in (False, True):
            eng = SearchEngine(_Spiked(smp, 4, col) if spiked else smp, OracleVerifier(), seed=seed)
            _, score, h = eng.fk_search(init, N, 0.5, [2], lam, potential=potential)
            res[potential, spiked] = (score, h, eng.best_image.clone())
    real = res["max", False][1]
    assert max(max(r) for r in real["trace_scores"]) < 0.999, "a real score reaches the spike"
    assert res["max", True][1]["parents"] == [[col] * N]
    assert real["parents"] != [[col] * N]
    assert res["max", True][1]["trace_scores"][1][col] == 1.0  # (row 4 is the window's second row)
    ds, dh, dimg = res["diff", True]
    rs, rh, rimg = res["diff", False]
    assert {k: v for k, v in dh.items() if k != "trace_scores"} == {k: v for k, v in rh.items() if k != "trace_scores"}
    assert ds == rs and torch.equal(dimg, rimg)
    assert dh["trace_scores"][0] == rh["trace_scores"][0] and dh["trace_scores"][2:] == rh["trace_scores"][2:]


def test_refusals(smp):
    eng = SearchEngine(smp, OracleVerifier(), seed=1)
    init = eng.initial_noise(SHAPE)
    for steps in ([], [5], [0], [2, 3], [3, 3], 3, [2.5]):
        with pytest.raises(ValueError, match="resample"):
            eng.fk_search(init, N, 0.5, steps, 1.0)
    with pytest.raises(ValueError, match="potential"):
        eng.fk_search(init, N, 0.5, [3], 1.0, potential="sum")
    with pytest.raises(ValueError, match="lam"):
        eng.fk_search(init, N, 0.5, [3], float("nan"))
    with pytest.raises(ValueError, match="trace_kind"):
        SearchEngine(smp, SelfSupervisedVerifier(), seed=1).fk_search(init, N, 0.5, [3], 1.0)
    with pytest.raises(ValueError, match="ddim"):
        SearchEngine(_sampler(ARCH_TINY), OracleVerifier(), seed=1).fk_search(init, N, 0.5, [3], 1.0)
    det = GaussianDiffusionSampler(smp.model, 1e-4, 0.02, T, sampler="ddim", steps=K, eta=0.0, clip_x0=True)
    with pytest.raises(ValueError, match="eta"):
        SearchEngine(det, OracleVerifier(), seed=1).fk_search(init, N, 0.5, [3], 1.0)


def test_product_class(smp):
    init = SearchEngine(smp, OracleVerifier(), seed=2).initial_noise(SHAPE)
    ps = ParticleSearch(n_particles=N, resample_steps=[4, 2], noise_scale=0.5, lam=300.0, potential="max")
    b, s, h = ps.search(init, None, OracleVerifier(), batched=True, sampler=smp, seed=2)
    eb, es, eh = SearchEngine(smp, OracleVerifier(), seed=2).fk_search(init, N, 0.5, [4, 2], 300.0, potential="max")
    assert h == eh and s == es and torch.equal(b, eb) and ps.nfes == N


def test_one_rank_nccl_group_equals_no_group():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fk_rccl_child.py"), str(port)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["backend"] == "nccl" and out["dist_with"] is True and out["dist_without"] is False
    assert out["identical"] is True and out["unet_steps"] == N * K and len(out["parents"]) == 2


def test_entry_particle(tmp_path):
    """search.algorithm: particle through load_config writes the best image and its JSON, and is the engine's call."""
    sd = synthetic_state_dict(ARCH_TINY, 5)
    torch.save(sd, str(tmp_path / "ckpt_0_.pt"))
    over = [f"save_weight_dir={tmp_path}", "test_load_weight=ckpt_0_.pt", "T=1000", f"inference_T={T}", "channel=32",
            "channel_mult=[1,2]", "attn=[1]", "num_res_blocks=1", "batch_size=2", "nrow=2", "seed=3",
            f"sampled_dir={tmp_path / 'out'}", "sampler.kind=ddim", f"sampler.steps={K}", "sampler.eta=1.0",
            "sampler.clip_x0=true", "search.algorithm=particle", f"search.n_particles={N}", "search.noise_scale=0.5",
            "search.resample_steps=[4,2]", "search.lam=300.0", "search.potential=max"]
    s = E.run(E.load_config(None, over))["search"]
    with open(tmp_path / "out" / "SearchBestImgs.json") as fh:
        js = json.load(fh)
    assert os.path.exists(tmp_path / "out" / "SearchBestImgs.png")
    assert js["algorithm"] == "particle" and js["history"]["parents"] == s["history"]["parents"]
    assert js["history"]["unet_steps"] == N * K and js["nfes"] == N and s["best_image"].shape == SHAPE
    net = UNet(1000, 32, [1, 2], [1], 1, 0.0).to(DEV)
    net.load_state_dict(sd)
    smp = GaussianDiffusionSampler(net, 1e-4, 0.02, T, sampler="ddim", steps=K, eta=1.0, clip_x0=True)
    eng = SearchEngine(smp, OracleVerifier(), seed=3)
    _, hs, hh = eng.fk_search(eng.initial_noise(SHAPE), N, 0.5, [4, 2], 300.0, potential="max")
    assert hh == s["history"] and hs == s["best_score"] and torch.equal(eng.best_image, s["best_image"])
    with pytest.raises(ValueError, match="search.potential"):
        E.run(E.load_config(None, [o.replace("potential=max", "potential=sum") for o in over]))
    with pytest.raises(ValueError, match=r"sampler\.(kind|eta)"):
        E.run(E.load_config(None, [o for o in over if not o.startswith("sampler.")]))
