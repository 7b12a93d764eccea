"""CPU checks of the guidance schedules: ``schedule.guidance_rows`` values, the ``guidance:`` / ``search.guidance_scales``
config validation, the engine's candidate -> multiplier assignment on a sampler stand-in (sharded and not), and the
host-side contract of itsd_set_guidance and the ``cfg_skip`` option. No GPU: every refusal here comes before any device
call. The refusals that need a UNet handle and the numerics are in tests/test_gpu_guidance.py."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from itsd import entry as E
from itsd import runtime as rt
from itsd.schedule import guidance_rows, strided_timesteps
from itsd.search import SearchEngine

TAU = [2, 5, 8, 11]


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ----------------------------------------------------------------------------- guidance_rows
def test_rows_constant():
    r = guidance_rows(TAU, 1.8, "constant")
    assert r.dtype == torch.float32 and r.shape == (4,) and torch.equal(r, _f32([1.8] * 4))
    assert torch.equal(guidance_rows(TAU, 1.8, {"kind": "constant"}), r)


def test_rows_interval_edges_fall_on_tau_entries():
    # both edges are timesteps of the schedule and are included
    assert torch.equal(guidance_rows(TAU, 1.8, {"kind": "interval", "t_lo": 5, "t_hi": 8}), _f32([0, 1.8, 1.8, 0]))
    # one past either edge drops that row
    assert torch.equal(guidance_rows(TAU, 1.8, {"kind": "interval", "t_lo": 6, "t_hi": 8}), _f32([0, 0, 1.8, 0]))
    assert torch.equal(guidance_rows(TAU, 1.8, {"kind": "interval", "t_lo": 5, "t_hi": 7}), _f32([0, 1.8, 0, 0]))
    assert torch.equal(guidance_rows(TAU, 1.8, {"kind": "interval", "t_lo": 0, "t_hi": 11}), _f32([1.8] * 4))
    assert torch.equal(guidance_rows(TAU, 1.8, {"kind": "interval", "t_lo": 3, "t_hi": 4}), _f32([0.0] * 4))
    assert torch.equal(guidance_rows(TAU, 1.8, {"kind": "interval", "t_lo": 11, "t_hi": 11}), _f32([0, 0, 0, 1.8]))


def test_rows_linear_runs_from_the_top_row_to_row_0():
    r = guidance_rows(TAU, 9.0, {"kind": "linear", "w_top": 3.0, "w_end": 0.0})  # (w itself is not read)
    assert torch.equal(r, _f32([0.0, 1.0, 2.0, 3.0]))
    r = guidance_rows(list(range(5)), 0.0, {"kind": "linear", "w_top": 0.5, "w_end": 2.5})
    assert torch.equal(r, _f32([2.5, 2.0, 1.5, 1.0, 0.5]))
    assert torch.equal(guidance_rows([7], 0.0, {"kind": "linear", "w_top": 0.5, "w_end": 2.5}), _f32([2.5]))


def test_rows_table():
    r = guidance_rows(TAU, 1.8, {"kind": "table", "values": [0.9, 1.8, 0.45, 1.8]})
    assert torch.equal(r, _f32([0.9, 1.8, 0.45, 1.8]))


@pytest.mark.parametrize("spec, key", [
    ({"kind": "ramp"}, r"guidance\.kind"),
    ({}, r"guidance\.kind"),
    ({"kind": "interval", "t_lo": 2}, r"guidance\.t_hi"),
    ({"kind": "interval", "t_lo": 2.5, "t_hi": 8}, r"guidance\.t_lo"),
    ({"kind": "interval", "t_lo": -1, "t_hi": 8}, r"guidance\.t_lo"),
    ({"kind": "interval", "t_lo": 9, "t_hi": 8}, r"guidance\.t_hi"),
    ({"kind": "interval", "t_lo": 2, "t_hi": True}, r"guidance\.t_hi"),
    ({"kind": "linear", "w_top": 1.0}, r"guidance\.w_end"),
    ({"kind": "linear", "w_top": float("nan"), "w_end": 0.0}, r"guidance\.w_top"),
    ({"kind": "linear", "w_top": 1.0, "w_end": "x"}, r"guidance\.w_end"),
    ({"kind": "table", "values": [1.0, 2.0, 3.0]}, r"guidance\.values"),
    ({"kind": "table", "values": [1.0, 2.0, 3.0, float("inf")]}, r"guidance\.values\[3\]"),
    ({"kind": "table", "values": 1.0}, r"guidance\.values"),
    ({"kind": "constant", "t_lo": 2}, r"guidance\.t_lo"),
    ({"kind": "table", "values": [1.0] * 4, "w_top": 2.0}, r"guidance\.w_top"),
])
def test_rows_bad_values_name_their_key(spec, key):
    with pytest.raises(ValueError, match=key):
        guidance_rows(TAU, 1.8, spec)


# ----------------------------------------------------------------------------- config
BASE = {"T": 12, "w": 1.8, "sampler": {"kind": "ddim", "steps": 4}}


def test_config_builds_the_rows_of_the_strided_schedule():
    assert strided_timesteps(12, 4) == TAU
    ga = E.guidance_args({**BASE, "guidance": {"kind": "interval", "t_lo": 5, "t_hi": 8},
                          "search": {"guidance_scales": [0.5, 1, 1.5]}}, 12)
    assert torch.equal(ga["guidance"], _f32([0, 1.8, 1.8, 0])) and ga["guidance_scales"] == [0.5, 1.0, 1.5]
    assert E.guidance_args(BASE, 12) == {"guidance": None, "guidance_scales": None}
    ga = E.guidance_args({**BASE, "sampler": {"kind": "dpmpp2m", "steps": 4}, "guidance": {"kind": "constant"}}, 12)
    assert torch.equal(ga["guidance"], _f32([1.8] * 4)) and ga["guidance_scales"] is None


@pytest.mark.parametrize("extra, key", [
    ({"guidance": {"kind": "nope"}}, r"guidance\.kind"),
    ({"guidance": "interval"}, r"guidance must be a block"),
    ({"guidance": {"kind": "interval", "t_lo": 5}}, r"guidance\.t_hi"),
    ({"guidance": {"kind": "table", "values": [1, 2]}}, r"guidance\.values"),
    ({"guidance": {"kind": "linear", "w_top": 1.0, "w_end": None}}, r"guidance\.w_end"),
    ({"search": {"guidance_scales": []}}, r"search\.guidance_scales"),
    ({"search": {"guidance_scales": 1.0}}, r"search\.guidance_scales"),
    ({"search": {"guidance_scales": [1.0, -0.5]}}, r"search\.guidance_scales"),
    ({"search": {"guidance_scales": [1.0, float("nan")]}}, r"search\.guidance_scales"),
    ({"search": {"guidance_scales": [1.0, True]}}, r"search\.guidance_scales"),
    ({"search": {"guidance_scales": [1.0, "2"]}}, r"search\.guidance_scales"),
])
def test_config_bad_values_name_their_key(extra, key):
    with pytest.raises(ValueError, match=key):
        E.guidance_args({**BASE, **extra}, 12)


@pytest.mark.parametrize("sampler", [None, {"kind": "ddpm"}])
def test_config_refuses_the_ancestral_sampler(sampler):
    cfg = {"T": 12, "w": 1.8, "guidance": {"kind": "constant"}}
    if sampler is not None:
        cfg["sampler"] = sampler
    with pytest.raises(ValueError, match=r"guidance needs sampler\.kind"):
        E.guidance_args(cfg, 12)
    cfg = {"T": 12, "w": 1.8, "search": {"guidance_scales": [1.0]}, **({} if sampler is None else {"sampler": sampler})}
    with pytest.raises(ValueError, match=r"search\.guidance_scales needs sampler\.kind"):
        E.guidance_args(cfg, 12)


def test_config_refused_under_main_py():
    """The unconditional entry (Main.py: ``run(cfg, condition=False)``) refuses both keys before anything is built."""
    for extra, key in (({"guidance": {"kind": "constant"}}, r"^guidance belongs"),
                       ({"search": {"guidance_scales": [1.0]}}, r"^search\.guidance_scales belongs")):
        cfg = E.load_config(None, ["state=eval"])
        cfg.update({"sampler": {"kind": "ddim", "steps": 4}})
        cfg.update(extra)
        with pytest.raises(ValueError, match=key):
            E.run(cfg, condition=False)


# ----------------------------------------------------------------------------- the engine on a stand-in
class _Model:
    device = torch.device("cpu")


class _Sampler:
    """The identity sampler; records what each run was given."""
    model = _Model()
    T = 4

    def __init__(self):
        self.runs = []

    def run(self, x, labels=None, seed=0, noise_offset=0, graph=True, **kw):
        self.runs.append(dict(kw, n=x.shape[0], noise_offset=noise_offset))
        return x


class _Verifier:
    kind = 0

    def score_batch(self, images, n_cand):
        return images.reshape(n_cand, -1).double().mean(dim=1)


class _Engine(SearchEngine):
    def candidate_noise(self, round_id, g0, count, shape, pivot=None, scale=1.0):
        g = torch.arange(g0, g0 + count, dtype=torch.float32).repeat_interleave(shape[0])
        return g.reshape(-1, 1, 1, 1).expand(-1, *shape[1:]).contiguous()  # candidate g scores g: the last one wins


SHAPE = (2, 3, 4, 4)  # batch_per_candidate = 2


def test_engine_deals_scales_by_global_index():
    scales = [0.5, 1.0, 1.5]
    smp = _Sampler()
    eng = _Engine(smp, _Verifier(), seed=1, guidance_scales=scales)
    _, score, h = eng.random_search(8, SHAPE)
    want = [scales[g % 3] for g in range(8)]
    (run,) = smp.runs
    gs = run["guidance_scale"]
    assert gs.dtype == torch.float32 and torch.equal(gs, _f32([w for w in want for _ in range(2)]))
    assert h["guidance_scales"] == want and h["best_index"] == 7 and h["best_guidance_scale"] == scales[7 % 3]
    # two ranks' shards are the unsharded assignment, cut in two
    parts = []
    for rank in range(2):
        s2 = _Sampler()
        e2 = _Engine(s2, _Verifier(), seed=1, guidance_scales=scales)
        e2.world, e2.rank = 2, rank
        e2.run_round(0, 8, SHAPE)
        assert s2.runs[0]["n"] == 8 and s2.runs[0]["noise_offset"] == rank * 4 * 2 * 48
        parts.append(s2.runs[0]["guidance_scale"])
    assert torch.equal(torch.cat(parts), gs)


def test_engine_without_scales_calls_the_sampler_as_before():
    smp = _Sampler()
    _, _, h = _Engine(smp, _Verifier(), seed=1).random_search(4, SHAPE)
    assert "guidance_scale" not in smp.runs[0] and set(h) == {"scores", "best_index"}


def test_engine_zero_order_and_path_report_the_best_scale():
    scales = [0.25, 2.0]
    eng = _Engine(_Sampler(), _Verifier(), seed=1, guidance_scales=scales)
    _, _, h = eng.zero_order_search(torch.zeros(SHAPE), 4, 0.9, 3)
    assert h["guidance_scales"] == [0.25, 2.0, 0.25, 2.0] and h["best_guidance_scale"] == 2.0  # candidate 3
    _, _, h = eng.path_search(torch.zeros(SHAPE), 3, 0.1)
    assert h["guidance_scales"] == [0.25, 2.0, 0.25] and h["best_guidance_scale"] == 0.25  # candidate 2
    assert all(torch.equal(r["guidance_scale"][:4], _f32([0.25, 0.25, 2.0, 2.0])) for r in eng.sampler.runs)


def test_engine_refuses_bad_scales_and_the_three_other_searches():
    for bad in ([], [1.0, -1.0], [float("inf")], [float("nan")]):
        with pytest.raises(ValueError, match="guidance_scales"):
            _Engine(_Sampler(), _Verifier(), guidance_scales=bad)
    eng = _Engine(_Sampler(), _Verifier(), seed=1, guidance_scales=[0.5, 1.0])
    init = torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError, match="path_search_branch does not take guidance_scales"):
        eng.path_search_branch(init, 4, 0.1, [2], keep=2)
    with pytest.raises(ValueError, match="fk_search does not take guidance_scales"):
        eng.fk_search(init, 4, 0.1, [2], 1.0)
    with pytest.raises(ValueError, match="gradient_search does not take guidance_scales"):
        eng.gradient_search(init, 2, 0.1, 2)
    assert eng.sampler.runs == []


# ----------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(rt.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return rt.lib()


def test_symbol_exported_bound_and_declared(L):
    lib = ctypes.CDLL(rt.LIB_PATH)
    assert hasattr(lib, "itsd_set_guidance"), "missing export itsd_set_guidance"
    assert "itsd_set_guidance" in rt.EXPORTS and hasattr(rt.NativeUNet, "set_guidance")
    src = open(os.path.join(ROOT, "include", "itsd.h")).read()
    assert re.search(r"^int\s+itsd_set_guidance\s*\(itsd_unet\* u, const float\* w_rows, int rows, "
                     r"const float\* w_img, int n_img\);", src, re.M)
    head = src[:src.index("#ifndef ITSD_H")]
    assert "itsd_set_guidance" in head, "the header comment cites every entry point"


@pytest.mark.parametrize("detach", [False, True])
def test_null_handle(L, detach):
    rows = (ctypes.c_float * 4)(0.0, 1.8, 1.8, 0.0)
    rc = L.itsd_set_guidance(None, None if detach else ctypes.cast(rows, ctypes.c_void_p), 4, None, 0)
    msg = L.itsd_last_error().decode()
    assert rc == rt.ITSD_ERR_INVALID and "itsd_set_guidance" in msg and "null handle" in msg


def test_cfg_skip_option(L):
    for v in (0, 1):
        rt.set_option("cfg_skip", v)
    assert L.itsd_set_option(b"cfg_skip", 2) == rt.ITSD_ERR_INVALID and "cfg_skip" in L.itsd_last_error().decode()
    with pytest.raises(rt.ItsdError):
        rt.set_option("cfg_skip", -1)
    rt.set_option("cfg_skip", 1)  # (a refused value left the previous setting; the shipped one is put back anyway)


def test_query_keys_refuse_a_null_handle(L):
    v = ctypes.c_int64(7)
    for key in (b"guidance", b"cond_only_steps"):
        assert L.itsd_unet_query(None, key, ctypes.byref(v)) == rt.ITSD_ERR_INVALID
