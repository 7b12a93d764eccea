"""Host-side contract of the model-as-verifier (itsd_verify_denoise, DenoisingVerifier): the entry point is exported,
bound and refuses a null handle before any device call; the default probe rows; the fp64 score combination against
hand values; and the engine's context rule -- labels go to a verifier that declares ``needs_context`` and to no other.
No GPU here: the kernels are covered by tests/test_gpu_verify_denoise.py."""
import ctypes
import os

import pytest
import torch

from itsd import entry as E
from itsd import runtime as rt
from itsd.search import SearchEngine
from itsd.verifier import VERIFIERS, DenoisingVerifier, combine_sse, probe_rows
from test_search_branch_cpu import CPUEngine, SHAPE, _Sampler, _Verifier


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def test_symbol_exported_and_bound(L):
    assert hasattr(ctypes.CDLL(rt.LIB_PATH), "itsd_verify_denoise")
    assert "itsd_verify_denoise" in rt.EXPORTS
    assert VERIFIERS["denoise"] is DenoisingVerifier and VERIFIERS["class"] is DenoisingVerifier
    assert DenoisingVerifier.kind == rt.VERIFY_DENOISE and DenoisingVerifier.needs_context is True


def test_null_arguments_refused_before_any_device_call(L):
    for u, x0, sse in ((None, 0x10000, 0x20000),):  # a null handle (the other nulls need a handle: the GPU test)
        rc = L.itsd_verify_denoise(u, x0, None, 1, 0, 1.0, 0.0, 0, 0, None, sse, None, None, None)
        assert rc == rt.ITSD_ERR_INVALID
        assert b"itsd_verify_denoise" in L.itsd_last_error()


@pytest.mark.parametrize("n_steps,R", [(1000, 4), (50, 4), (4, 4), (12, 1)])
def test_probe_rows_increasing_and_in_range(n_steps, R):
    rows = probe_rows(n_steps, R)
    assert len(rows) == R and all(0 <= r < n_steps for r in rows)
    assert all(b > a for a, b in zip(rows, rows[1:]))
    assert rows == [((2 * k + 1) * n_steps) // (2 * R) for k in range(R)]


def test_probe_rows_values_and_refusals():
    assert probe_rows(1000, 4) == [125, 375, 625, 875]
    assert probe_rows(4, 4) == [0, 1, 2, 3] and probe_rows(12, 1) == [6]
    for n_steps, R in ((4, 5), (4, 0)):
        with pytest.raises(ValueError):
            probe_rows(n_steps, R)


def test_score_combination_hand_values():
    # 2 probes, 4 images (2 candidates of 2), P = 8 elements an image; every value a small power-of-two multiple,
    # so the fp64 arithmetic below is exact and the comparison is equality
    sse = torch.tensor([[[8.0, 16.0], [4.0, 4.0], [0.0, 8.0], [16.0, 8.0]],
                        [[24.0, 16.0], [4.0, 12.0], [8.0, 8.0], [0.0, 24.0]]], dtype=torch.float64)
    # denoise: -mean_r sse_c / P per image = -(16, 4, 4, 8) / 8 = (-2, -.5, -.5, -1); candidates (-1.25, -0.75)
    assert combine_sse(sse, "denoise", 8, 2).tolist() == [-1.25, -0.75]
    # class: mean_r (sse_u - sse_c) / P per image = ((8 - 8) / 2, (0 + 8) / 2, (8 + 0) / 2, (-8 + 24) / 2) / 8
    #        = (0, .5, .5, 1); candidates (0.25, 0.75)
    assert combine_sse(sse, "class", 8, 2).tolist() == [0.25, 0.75]
    assert combine_sse(sse, "class", 8, 4).tolist() == [0.0, 0.5, 0.5, 1.0]
    out = combine_sse(sse.float(), "denoise", 8, 1)
    assert out.dtype == torch.float64 and out.tolist() == [-1.0]
    nan = sse.clone()
    nan[1, 2, 0] = float("nan")  # a NaN error sum stays a NaN score of that candidate only
    got = combine_sse(nan, "denoise", 8, 2)
    assert got[0].item() == -1.25 and torch.isnan(got[1])


class _Plain(_Verifier):
    """No needs_context: the two-argument call, as every verifier before this one."""

    def __init__(self):
        self.calls = []

    def score_batch(self, images, n_cand):  # (a labels= keyword would be a TypeError)
        self.calls.append(n_cand)
        return super().score_batch(images, n_cand)


class _Context(_Verifier):
    needs_context = True
    probes = 3

    def __init__(self):
        self.labels = []

    def score_batch(self, images, n_cand, labels=None):
        self.labels.append(None if labels is None else labels.clone())
        return super().score_batch(images, n_cand)


def test_engine_passes_context_only_where_declared():
    lab = torch.tensor([5], dtype=torch.int32)
    plain, ctx = _Plain(), _Context()
    e0 = CPUEngine(_Sampler(), plain, seed=3)
    _, s0, h0 = e0.path_search_branch(torch.zeros(SHAPE), 8, 0.5, [8, 3], keep=2, renoise_steps=2, labels=lab)
    assert plain.calls == [8, 8, 8] and "verifier_unet_steps" not in h0
    e1 = CPUEngine(_Sampler(), ctx, seed=3)
    _, s1, h1 = e1.path_search_branch(torch.zeros(SHAPE), 8, 0.5, [8, 3], keep=2, renoise_steps=2, labels=lab)
    # the repeated labels of the round at every scoring site: two stages and the final scores
    assert len(ctx.labels) == 3 and all(torch.equal(v, lab.repeat(8)) for v in ctx.labels)
    assert h1["verifier_unet_steps"] == 3 * 8 * 3
    assert s0 == s1 and {k: v for k, v in h1.items() if k != "verifier_unet_steps"} == h0
    # the single-round searches: the same rule, and the counter starts over with each search
    _, _, h = e1.path_search(torch.zeros(SHAPE), 4, 0.5, 400, labels=lab)
    assert h["verifier_unet_steps"] == 4 * 3 and torch.equal(ctx.labels[-1], lab.repeat(4))
    _, _, h = e1.zero_order_search(torch.zeros(SHAPE), 4, 0.95, 2)
    assert h["verifier_unet_steps"] == 2 * 4 * 3 and ctx.labels[-1] is None
    _, _, h = e0.path_search(torch.zeros(SHAPE), 4, 0.5, 400, labels=lab)
    assert set(h) == {"scores", "injection_points", "best_index"}


class _Arch:
    def __init__(self, cfg):
        self.cfg = cfg


class _Net:
    device = torch.device("cpu")

    def __init__(self, cfg):
        self.arch = _Arch(cfg)


def _stub_sampler(cfg, sampler="ddpm", steps=None):
    from itsd.diffusion import GaussianDiffusionSampler

    kw = {} if sampler == "ddpm" else {"sampler": "ddim", "steps": steps}
    return GaussianDiffusionSampler(_Net(cfg), 1e-4, 0.02, 1000, **kw)


def test_verifier_construction():
    v = DenoisingVerifier(_stub_sampler(False))
    assert v.rows == [125, 375, 625, 875] and v.probes == 4 and v.mode == "denoise"
    abar = v.sampler.sched.alphas_bar.double()
    for (a, b), r in zip(v.ab, v.rows):  # sqrt(abar), sqrt(1 - abar) of the row, fp64
        assert a == float(torch.sqrt(abar[r])) and b == float(torch.sqrt(1.0 - abar[r]))
        assert abs(a * a + b * b - 1.0) < 1e-15
    # under a few-step sampler the rows are rows of ITS schedule, and abar is tau's
    d = DenoisingVerifier(_stub_sampler(True, "ddim", 50), mode="class", probes=[0, 49])
    assert d.rows == [0, 49] and d.sampler.n_steps == 50
    assert d.ab[1][0] == float(torch.sqrt(d.sampler.sched.alphas_bar.double()[d.sampler.tau[49]]))
    assert DenoisingVerifier(_stub_sampler(True, "ddim", 50)).rows == probe_rows(50, 4)
    with pytest.raises(ValueError, match="class"):
        DenoisingVerifier(_stub_sampler(False), mode="class")
    with pytest.raises(ValueError):
        DenoisingVerifier(_stub_sampler(False), mode="clip")
    with pytest.raises(ValueError):
        DenoisingVerifier(_stub_sampler(True, "ddim", 50), probes=[50])
    with pytest.raises(ValueError):
        DenoisingVerifier(_stub_sampler(False), probes=[])


def test_entry_verifier_keys():
    smp, cond = _stub_sampler(False), _stub_sampler(True)
    v = E.search_verifier({"verifier": "denoise", "verifier_probes": 2, "verifier_seed": 9}, smp, False)
    assert isinstance(v, DenoisingVerifier) and v.rows == [250, 750] and v.seed == 9 and v.mode == "denoise"
    v = E.search_verifier({"verifier": "class", "verifier_probes": [3, 500]}, cond, True)
    assert v.mode == "class" and v.rows == [3, 500] and v.seed == 0
    assert type(E.search_verifier({}, smp, False)).__name__ == "OracleVerifier"
    with pytest.raises(ValueError, match="search.verifier"):
        E.search_verifier({"verifier": "class"}, cond, False)
    with pytest.raises(ValueError, match="search.verifier_probes"):
        E.search_verifier({"verifier": "denoise", "verifier_probes": 0}, smp, False)
    with pytest.raises(ValueError, match="search.verifier_probes"):
        E.search_verifier({"verifier": "denoise", "verifier_probes": [1000]}, smp, False)
    with pytest.raises(ValueError, match="search.verifier_seed"):
        E.search_verifier({"verifier": "denoise", "verifier_seed": -1}, smp, False)
    with pytest.raises(ValueError, match="search.verifier_probes"):
        E.search_verifier({"verifier": "oracle", "verifier_probes": 2}, smp, False)
    with pytest.raises(ValueError, match="search.verifier"):
        E.search_verifier({"verifier": "clip"}, smp, False)


def test_engine_accepts_the_verifier():
    eng = SearchEngine(_Sampler(), DenoisingVerifier(_stub_sampler(False)), seed=0)
    assert eng.verifier.needs_context and eng.verifier_unet_steps == 0
