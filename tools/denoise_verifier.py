"""Cost and score spread of the model-as-verifier: the Arch A bf16 UNet with the benchmark's seeded
synthetic weights. Measurement tool, never part of the product.

    python tools/denoise_verifier.py cost --n 256 [--reps 20] [--rounds 5]
        one eager probe (itsd_verify_denoise: noising kernel, the step's program, the sse tail, the finalize) next to
        the graph-replayed ancestral step at the same batch, interleaved, ms each (best / median of the rounds)
    python tools/denoise_verifier.py spread [--n 64] [--probes 4] [--out FILE.json]
        one random-search round of N candidates through the few-step sampler (ddim K = 50, eta = 1, clip on: the one
        whose images are not all rails), scored by DenoisingVerifier(mode="denoise") and by the Oracle verifier: max -
        min, top-2 gap and std of the N scores, per-probe mean error, and the scoring wall time
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from itsd.arch import ARCH_A
from itsd.diffusion import GaussianDiffusionSampler
from itsd.model import UNet
from itsd.search import SearchEngine
from itsd.verifier import DenoisingVerifier, OracleVerifier


def _net():
    a = ARCH_A
    return UNet(a.T, a.ch, a.ch_mult, a.attn, a.num_res_blocks, 0.0, img_size=32, precision="bf16", weights="gauss",
                seed=0).to("cuda:0")


def _timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(reps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def cost(args):
    smp = GaussianDiffusionSampler(_net(), 1e-4, 0.02, 1000)
    ver = DenoisingVerifier(smp, probes=[500])
    x = torch.randn(args.n, 3, 32, 32, device="cuda").clamp(-1, 1)
    nat = smp._native(args.n)
    sse = torch.empty(args.n, 2, dtype=torch.float64, device="cuda")
    (a, b), row = ver.ab[0], ver.rows[0]

    def probe(reps):
        for _ in range(reps):
            nat.verify_denoise(x, row, a, b, 0, 0xD0000000, sse=sse)

    def step(reps):
        smp.run(x.clone(), t_begin=999, t_end=999 - reps + 1, seed=1)

    probe(3)
    step(5)  # capture + warm
    res = {"probe": [], "step": []}
    for r in range(args.rounds):
        for name, fn in (("step", step), ("probe", probe)):
            ms = _timed(fn, args.reps)
            res[name].append(ms)
            print(f"round {r} n={args.n} {name}: {ms:.4f} ms", flush=True)
    for name, v in res.items():
        print(f"n={args.n} {name}: best {min(v):.4f} median {statistics.median(v):.4f} ms")
    print(f"n={args.n} probe / step: best {min(res['probe']) / min(res['step']):.3f} "
          f"median {statistics.median(res['probe']) / statistics.median(res['step']):.3f}")


def _stats(sc):
    s = torch.sort(sc, descending=True).values
    return {"score_max": float(s[0]), "score_min": float(s[-1]), "score_range": float(s[0] - s[-1]),
            "top2_gap": float(s[0] - s[1]), "score_std": float(sc.std()), "argmax": int(torch.argmax(sc))}


def spread(args):
    smp = GaussianDiffusionSampler(_net(), 1e-4, 0.02, 1000, sampler="ddim", steps=50, eta=1.0, clip_x0=True)
    ver = DenoisingVerifier(smp, mode="denoise", probes=args.probes, seed=args.seed)
    eng = SearchEngine(smp, ver, seed=args.seed)
    x = eng.candidate_noise(0, 0, args.n, (1, 3, 32, 32))
    smp.run(x, seed=(eng.seed * 1000003) & ((1 << 62) - 1), noise_offset=0)
    rec = {"sampler": "ddim K=50 eta=1 clip on", "n": args.n, "rows": ver.rows,
           "saturated_share": float((x.abs() >= 1.0).float().mean())}
    for timed in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = ver.score_batch(x, args.n).cpu()
        rec["denoise_wall_s"] = time.perf_counter() - t0
    rec["denoise"] = _stats(sc)
    nat, P = smp._native(args.n), x[0].numel()
    rec["mean_sq_error_per_probe"] = [
        float(nat.verify_denoise(x, row, a, b, ver.seed, 0xD0000000 + r)[:, 0].mean()) / P
        for r, (row, (a, b)) in enumerate(zip(ver.rows, ver.ab))]
    osc = OracleVerifier().score_batch(x, args.n).cpu()
    rec["oracle"] = _stats(osc)
    so, sd = osc - osc.mean(), sc - sc.mean()
    rec["pearson_denoise_vs_oracle"] = float((so * sd).sum() / (so.norm() * sd.norm()))
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "spread"])
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--probes", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    (cost if args.what == "cost" else spread)(args)


if __name__ == "__main__":
    main()
