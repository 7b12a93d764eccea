"""The stage loop of the branching path search (SearchEngine.path_search_branch) on CPU stand-ins: ranking, the parent
table, lineage and step bookkeeping, the refusals, and the world-size-2 gloo protocol (two collectives a stage) against
the single-process run. The stand-in sampler implements the windowed interface the engine uses -- run(t_begin..t_end),
predict_x0, T, sched -- with noise that is a pure function of (key, step, global position), as the native sampler's;
the engine's two device hooks, candidate_noise and branch_latents, are overridden the same way. The GPU path is
covered by tests/test_gpu_path_branch.py."""
import os
import socket
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from itsd.schedule import make_schedule, x0_coeffs
from itsd.search import (PathSearch, SearchEngine, branch_parents, default_keep, injection_step_list, rank_desc,
                         root_of, strict_argmax)

T = 12
NAN = float("nan")


def _hash_noise(key, step, start, count):
    """Deterministic pseudo-noise in [-1, 1) of global element positions start..start+count-1."""
    i = torch.arange(start, start + count, dtype=torch.float64)
    v = torch.sin(i * 12.9898 + step * 78.233 + (key % 9973) * 0.37) * 43758.5453
    return ((v - torch.floor(v)) * 2 - 1).float()


class _Model:
    device = torch.device("cpu")


class _Sampler:
    model = _Model()
    T = T

    def __init__(self):
        self.sched = make_schedule(1e-4, 0.02, T)
        self.windows = []  # (t_begin, t_end, seed, clip) of every run call

    def run(self, x, t_begin=None, t_end=0, labels=None, seed=0, noise_offset=0, graph=True, clip=None):
        t_begin = self.T - 1 if t_begin is None else t_begin
        clip = t_end == 0 if clip is None else clip
        self.windows.append((t_begin, t_end, seed, clip))
        for t in range(t_begin, t_end - 1, -1):
            z = _hash_noise(seed, t, noise_offset, x.numel()).view_as(x) if t > 0 else 0
            x.copy_(0.95 * torch.tanh(x * 1.1) + 0.2 * z)
        if clip:
            x.clamp_(-1, 1)
        return x

    def predict_x0(self, x, t, labels=None):
        a0, b0 = x0_coeffs(self.sched.alphas_bar, t)
        return (a0 * x - b0 * torch.tanh(x)).clamp(-1, 1)


class _Verifier:
    kind = 0

    def score_batch(self, images, n_cand):
        v = images.reshape(n_cand, -1).double()
        return 1.0 / (1.0 + v.var(dim=1))


class CPUEngine(SearchEngine):
    def candidate_noise(self, round_id, g0, count, shape, pivot=None, scale=1.0):
        outs = []
        for g in range(g0, g0 + count):
            gen = torch.Generator().manual_seed(self.seed * 1_000_003 + round_id * 10_007 + g)
            outs.append(torch.randn(shape, generator=gen) * scale + (pivot if pivot is not None else 0))
        return torch.cat(outs)

    def branch_latents(self, dst, src, parents, a, b, stage, cand_offset):
        per = dst.numel() // len(parents)
        s, d = src.reshape(-1, per), dst.view(-1, per)
        for j, p in enumerate(parents):
            d[j] = a * s[p] + b * _hash_noise(self.seed + 77, 1000 + stage, (cand_offset + j) * per, per)
        return dst


SHAPE = (1, 3, 4, 4)


def _search(eng, **kw):
    args = dict(n_paths=8, noise_scale=0.5, injection_steps=[8, 3], keep=2, renoise_steps=2)
    args.update(kw)
    return eng.path_search_branch(torch.zeros(SHAPE), **args)


# ----------------------------------------------------------------------------- ranking and tables
def test_rank_desc_ties_nan_all_nan():
    assert rank_desc(torch.tensor([0.1, NAN, 0.3, 0.3], dtype=torch.float64)) == [2, 3, 0, 1]
    assert rank_desc(torch.tensor([1.0, 1.0, 1.0])) == [0, 1, 2]
    assert rank_desc(torch.tensor([NAN, NAN, NAN])) == [0, 1, 2]
    assert rank_desc(torch.tensor([NAN, float("-inf"), 0.0])) == [2, 0, 1]  # NaN counts as -inf: index order
    # the head of the ranking is strict_argmax's winner
    sc = torch.tensor([0.2, 0.9, NAN, 0.9, -1.0], dtype=torch.float64)
    assert rank_desc(sc)[0] == strict_argmax(sc)[0] == 1


def test_parent_table_n8_keep2():
    sc = torch.tensor([0.1, 0.5, 0.3, 0.2, 0.9, 0.0, 0.7, 0.4], dtype=torch.float64)
    assert branch_parents(sc, 2) == [4, 4, 4, 4, 6, 6, 6, 6]
    assert branch_parents(sc, 8) == [4, 6, 1, 7, 2, 3, 0, 5]
    assert branch_parents(torch.arange(8, 0, -1).double(), 8) == list(range(8))  # descending scores: the identity
    with pytest.raises(ValueError):
        branch_parents(sc, 3)
    assert default_keep(8) == 2 and default_keep(4) == 1 and default_keep(12) == 3 and default_keep(10) == 2
    assert default_keep(14) == 2 and default_keep(3) == 1  # rounded down to a divisor
    assert injection_step_list(400) == [400] and injection_step_list([8, 3]) == [8, 3]


def test_root_of_lineage():
    parents = [[4, 4, 4, 4, 6, 6, 6, 6], [5, 5, 5, 5, 0, 0, 0, 0]]
    assert root_of(parents, 2) == 6    # 2 <- 5 (stage 1) <- 6 (stage 0)
    assert root_of(parents, 7) == 4    # 7 <- 0 <- 4
    assert root_of(parents, -1) == -1  # no winner
    assert root_of([], 3) == 3


# ----------------------------------------------------------------------------- the stage loop
def test_two_stage_bookkeeping_and_windows():
    smp = _Sampler()
    eng = CPUEngine(smp, _Verifier(), seed=3)
    best, score, h = _search(eng)
    assert h["injection_points"] == [8, 3]
    assert len(h["stage_scores"]) == 2 and all(len(s) == 8 for s in h["stage_scores"])
    for sc, tab in zip(h["stage_scores"], h["parents"]):
        assert tab == branch_parents(torch.tensor(sc, dtype=torch.float64), 2)
    assert h["best_index"] == strict_argmax(torch.tensor(h["scores"], dtype=torch.float64))[0]
    assert score == h["scores"][h["best_index"]]
    assert h["root_index"] == h["parents"][0][h["parents"][1][h["best_index"]]]
    # best_noise is the ROOT ancestor's initial candidate
    assert torch.equal(best, eng.candidate_noise(0, h["root_index"], 1, SHAPE, torch.zeros(SHAPE), 0.5))
    # windows: 11..9 (no clip) | branch at 8, re-noised to 10 | 10..4 | branch at 3, re-noised to 5 | 5..0 (clip)
    k = [eng.window_key(i, 2) for i in range(3)]
    assert smp.windows == [(11, 9, k[0], False), (10, 4, k[1], False), (5, 0, k[2], True)]
    assert len(set(k)) == 3 and k[0] == (3 * 1000003) & ((1 << 62) - 1)  # window 0: the placeholder round's key
    assert h["unet_steps"] == 8 * ((3 + 7 + 6) + 2)
    assert eng.nfes == 8  # the reference's unit: one per path
    # the kept image is the scored one
    assert abs(_Verifier().score_batch(eng.best_image, 1).item() - score) < 1e-12


def test_unet_steps_arithmetic():
    for steps, delta, want in [([8, 3], 0, (3 + 5 + 4) + 2), ([11], 0, (0 + 12) + 1), ([5], 6, (6 + 12) + 1),
                               ([9, 8, 1], 1, (2 + 2 + 8 + 3) + 3)]:
        eng = CPUEngine(_Sampler(), _Verifier(), seed=1)
        _, _, h = _search(eng, injection_steps=steps, renoise_steps=delta, n_paths=4, keep=2)
        assert h["unet_steps"] == 4 * want, (steps, delta)


def test_first_step_at_T_minus_1_skips_the_empty_window():
    smp = _Sampler()
    eng = CPUEngine(smp, _Verifier(), seed=1)
    _search(eng, injection_steps=[T - 1], renoise_steps=0)
    assert smp.windows == [(T - 1, 0, eng.window_key(0), True)]  # renoise_steps 0: the key never changes


def test_noop_stage_is_the_placeholder_round():
    """keep = N with descending stage scores makes every path its own only child, renoise_steps = 0 copies it: the
    search is then the placeholder round split into two windows."""
    class Descending(_Verifier):
        calls = 0

        def score_batch(self, images, n_cand):
            self.calls += 1
            if self.calls == 1:
                return torch.arange(n_cand, 0, -1, dtype=torch.float64)
            return super().score_batch(images, n_cand)

    init = torch.full(SHAPE, 0.25)
    ref = CPUEngine(_Sampler(), _Verifier(), seed=5)
    rb, rs, rh = ref.path_search(init, 4, 0.3, 400)
    eng = CPUEngine(_Sampler(), Descending(), seed=5)
    b, s, h = eng.path_search_branch(init, 4, 0.3, [6], keep=4, renoise_steps=0)
    assert h["parents"] == [[0, 1, 2, 3]]
    assert h["scores"] == rh["scores"] and h["best_index"] == rh["best_index"] and s == rs
    assert torch.equal(b, rb) and torch.equal(eng.best_image, ref.best_image)


def test_all_nan_final_scores_keep_the_initial_noise():
    class NaNVerifier(_Verifier):
        def score_batch(self, images, n_cand):
            return torch.full((n_cand,), NAN, dtype=torch.float64)

    eng = CPUEngine(_Sampler(), NaNVerifier(), seed=0)
    init = torch.ones(SHAPE)
    b, s, h = eng.path_search_branch(init, 4, 0.1, [5], keep=2)
    assert torch.equal(b, init) and s == float("-inf") and h["best_index"] == -1 and h["root_index"] == -1
    assert h["parents"] == [[0, 0, 1, 1]]  # all-NaN stage: index order


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [
    dict(injection_steps=[3, 8]),             # increasing
    dict(injection_steps=[8, 8]),             # not strictly decreasing
    dict(injection_steps=[]),                 # empty
    dict(injection_steps=8),                  # not a list
    dict(injection_steps=[8, 0]),             # s < 1
    dict(injection_steps=[10], renoise_steps=2),  # s + delta > T - 1
    dict(injection_steps=[T]),                # s > T - 1
    dict(renoise_steps=-1),
    dict(keep=3),                             # N % keep != 0
    dict(keep=0),
])
def test_refusals(kw):
    smp = _Sampler()
    eng = CPUEngine(smp, _Verifier(), seed=0)
    with pytest.raises(ValueError):
        _search(eng, **kw)
    assert smp.windows == [] and eng.nfes == 0  # refused before any work


def test_branch_mode_needs_batched():
    ps = PathSearch(n_paths=4, injection_step=[8, 3], noise_scale=0.1, mode="branch", keep=2)
    with pytest.raises(ValueError, match="batched"):
        ps.search(torch.zeros(SHAPE), lambda x, **k: x, lambda x, **k: 0.0, batched=False)
    with pytest.raises(ValueError):
        PathSearch(mode="tree")
    with pytest.raises(TypeError):
        PathSearch(4, 400, 0.1, False, "branch")  # the new parameters are keyword-only
    p = PathSearch()
    assert (p.mode, p.keep, p.renoise_steps, p.injection_step) == ("placeholder", None, 0, 400)


# ----------------------------------------------------------------------------- sharded
def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = CPUEngine(_Sampler(), _Verifier(), seed=3)
    best, score, h = _search(eng)
    torch.save({"best": best, "score": score, "hist": h, "image": eng.best_image.clone()}, f"{out_path}.{rank}")
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world2_equals_single_process():
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "res")
        mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
        rs = [torch.load(f"{out}.{r}", weights_only=False) for r in (0, 1)]
    single = CPUEngine(_Sampler(), _Verifier(), seed=3)
    best, score, h = _search(single)
    for r in rs:
        assert r["hist"]["scores"] == h["scores"] and r["hist"]["stage_scores"] == h["stage_scores"]
        assert r["hist"]["parents"] == h["parents"]
        assert r["hist"]["best_index"] == h["best_index"] and r["hist"]["root_index"] == h["root_index"]
        assert r["hist"]["unet_steps"] == h["unet_steps"] and r["score"] == score
        assert torch.equal(r["image"], single.best_image) and torch.equal(r["best"], best)
