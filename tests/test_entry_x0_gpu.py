"""The ``sampler:`` config block through the eval entry points (Main.py / MainCondition.py surface) on tiny UNets:
with the block the saved tensor is the few-step sampler class called directly; without it, the ancestral one, as
before. The entry against the same itsd components run by hand (the numerics underneath are pinned in
test_gpu_sampler_x0.py)."""
import dataclasses

import pytest
import torch

from itsd import entry as E
from itsd.arch import ARCH_TINY, ARCH_TINY_CFG
from itsd.diffusion import CondGaussianDiffusionSampler, GaussianDiffusionSampler
from itsd.model import CondUNet, UNet
from itsd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

BLOCK = ["sampler.kind=ddim", "sampler.steps=4", "sampler.eta=0.5", "sampler.clip_x0=true"]
KW = dict(sampler="ddim", steps=4, eta=0.5, clip_x0=True)


def test_main_eval_with_sampler_block(tmp_path):
    sd = synthetic_state_dict(ARCH_TINY, 5)
    torch.save(sd, str(tmp_path / "ckpt_0_.pt"))
    base = [f"save_weight_dir={tmp_path}", "test_load_weight=ckpt_0_.pt", "T=1000", "inference_T=12", "channel=32",
            "channel_mult=[1,2]", "attn=[1]", "num_res_blocks=1", "batch_size=4", f"sampled_dir={tmp_path}/out",
            "nrow=2", "seed=3"]
    res = E.run(E.load_config(None, base + BLOCK + ["search.algorithm=random", "search.n_candidates=4"]))
    plain = E.run(E.load_config(None, base))

    def by_hand(**kw):  # the entry's order: seed, model, x_T draw on the device, sampler (its Philox seed: CPU generator)
        torch.manual_seed(3)
        net = UNet(1000, 32, [1, 2], [1], 1, 0.0).to("cuda:0")
        net.load_state_dict(sd)
        x = torch.randn(4, 3, 32, 32, device="cuda:0")
        smp = GaussianDiffusionSampler(net, 1e-4, 0.02, 12, **kw)
        return x, smp, smp(x) * 0.5 + 0.5

    x, _, ref = by_hand()
    assert torch.equal(x, plain["noisy"]) and torch.equal(ref, plain["sampled"])
    x, smp, ref = by_hand(**KW)
    assert smp.n_steps == 4
    assert torch.equal(x, res["noisy"]) and torch.equal(ref, res["sampled"])
    assert not torch.equal(res["sampled"], plain["sampled"])
    # the search block's rounds run the same few-step sampler
    from itsd.search import SearchEngine
    from itsd.verifier import OracleVerifier

    _, score, h = SearchEngine(smp, OracleVerifier(), seed=3).random_search(4, (1, 3, 32, 32))
    assert res["search"]["history"] == h and res["search"]["best_score"] == score
    with pytest.raises(ValueError, match=r"sampler\.steps"):
        E.run(E.load_config(None, base + ["sampler.kind=ddim", "sampler.steps=13"]))


def test_main_condition_eval_with_sampler_block(tmp_path):
    a = dataclasses.replace(ARCH_TINY_CFG, T=12)  # the CFG time table has T rows
    sd = synthetic_state_dict(a, 6)
    torch.save(sd, str(tmp_path / "ckpt_63_.pt"))
    base = [f"save_dir={tmp_path}", "test_load_weight=ckpt_63_.pt", "T=12", "channel=32", "channel_mult=[1,2]",
            "num_res_blocks=1", "batch_size=10", f"sampled_dir={tmp_path}", "seed=1"]
    res = E.run(E.load_config(None, base + BLOCK, config_name="condition_config"), condition=True)
    plain = E.run(E.load_config(None, base, config_name="condition_config"), condition=True)

    def by_hand(**kw):
        torch.manual_seed(1)
        net = CondUNet(12, 10, 32, [1, 2], 1, 0.0).to("cuda:0")
        net.load_state_dict(sd)
        x = torch.randn(10, 3, 32, 32, device="cuda:0")
        return x, CondGaussianDiffusionSampler(net, 1e-4, 0.028, 12, w=1.8, **kw)(x, res["labels"]) * 0.5 + 0.5

    x, ref = by_hand(**KW)
    assert torch.equal(x, res["noisy"]) and torch.equal(ref, res["sampled"])
    x, ref = by_hand()
    assert torch.equal(ref, plain["sampled"]) and not torch.equal(res["sampled"], plain["sampled"])
