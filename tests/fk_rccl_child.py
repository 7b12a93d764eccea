"""Child process of tests/test_gpu_fk_search.py (not a test module): runs SearchEngine.fk_search under a one-rank RCCL
("nccl") process group -- the stage's all_gather of the window's trace scores, the final all_gather and the
winner-image broadcast really execute on the GPU -- then the same search with no process group, and prints one JSON
line comparing them. Started in a fresh process so that the process group is initialised before anything touches the
GPU (as tests/rccl_child.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist


def search():
    from itsd.arch import ARCH_TINY
    from itsd.diffusion import GaussianDiffusionSampler
    from itsd.model import UNet
    from itsd.search import SearchEngine
    from itsd.verifier import OracleVerifier

    a = ARCH_TINY
    net = UNet(a.T, a.ch, a.ch_mult, a.attn, a.num_res_blocks, 0.0, precision="fp32", device="cuda:0")
    smp = GaussianDiffusionSampler(net, 1e-4, 0.02, 12, sampler="ddim", steps=6, eta=1.0, clip_x0=True)
    eng = SearchEngine(smp, OracleVerifier(), seed=21)
    init = eng.initial_noise((1, 3, 32, 32))
    bn, bs, h = eng.fk_search(init, 8, 0.5, [4, 2], 300.0, potential="max")
    out = {"dist": eng.dist, "hist": h, "best_score": bs, "best_noise": bn.cpu().flatten().tolist()[:64],
           "best_image": eng.best_image.cpu().flatten().tolist()[:64]}
    del eng, smp, net
    torch.cuda.empty_cache()
    return out


def main():
    port = sys.argv[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    backend = dist.get_backend()
    with_group = search()
    dist.barrier()
    dist.destroy_process_group()
    without = search()
    same = all(with_group[k] == without[k] for k in ("hist", "best_score", "best_noise", "best_image"))
    print(json.dumps({"backend": backend, "dist_with": with_group["dist"], "dist_without": without["dist"],
                      "identical": same, "parents": with_group["hist"]["parents"],
                      "unet_steps": with_group["hist"]["unet_steps"]}), flush=True)


if __name__ == "__main__":
    main()
