"""Score spread of one random-search round under the ancestral and the few-step samplers: the
Arch A bf16 UNet with the seeded synthetic weights, N candidates, the Oracle verifier. For each sampler: max |x|
before the final clip, the share of saturated pixels after it, max - min and the top-2 gap of the N scores, and the
wall time of the round. Measurement tool, never part of the product.

    python tools/score_spread.py [--n 64] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from itsd.arch import ARCH_A
from itsd.diffusion import GaussianDiffusionSampler
from itsd.model import UNet
from itsd.search import SearchEngine
from itsd.verifier import OracleVerifier

CASES = [("ddpm T=1000", {}),
         ("ddim K=50 eta=0 clip off", dict(sampler="ddim", steps=50, eta=0.0, clip_x0=False)),
         ("ddim K=50 eta=1 clip on", dict(sampler="ddim", steps=50, eta=1.0, clip_x0=True)),
         ("ddim K=1000 eta=1 clip on", dict(sampler="ddim", steps=1000, eta=1.0, clip_x0=True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    a = ARCH_A
    net = UNet(a.T, a.ch, a.ch_mult, a.attn, a.num_res_blocks, 0.0, img_size=32, precision="bf16", weights="gauss",
               seed=0).to("cuda:0")  # the benchmark's weights
    shape, ver, rows = (1, 3, 32, 32), OracleVerifier(), []
    for name, kw in CASES:
        smp = GaussianDiffusionSampler(net, 1e-4, 0.02, 1000, **kw)
        eng = SearchEngine(smp, ver, seed=args.seed)
        rec = {"sampler": name, "n": args.n, "rows": smp.n_steps}
        for timed in (False, True):  # the first pass captures the step graph
            x = eng.candidate_noise(0, 0, args.n, shape)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:  # the round's own key and offsets (SearchEngine.run_round), the final clip taken apart
                smp.run(x, seed=(eng.seed * 1000003) & ((1 << 62) - 1), noise_offset=0, clip=False)
            except AssertionError as e:  # the sampler's NaN flag
                rec["error"] = str(e)
            sc = ver.score_batch(x.clamp(-1.0, 1.0), args.n).cpu()
            rec["wall_s"] = time.perf_counter() - t0
        s = torch.sort(sc, descending=True).values
        rec.update({"max_abs_x_before_clip": float(x.abs().max()), "nan_elements": int(torch.isnan(x).sum()),
                    "saturated_share": float((x.abs() >= 1.0).float().mean()),
                    "score_max": float(s[0]), "score_min": float(s[-1]), "score_range": float(s[0] - s[-1]),
                    "top2_gap": float(s[0] - s[1]), "score_std": float(sc.std())})
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
