"""A/B of itsd_set_option settings on the graph-replayed sampler step (the bench's timed path), in one
process, interleaved. Measurement tool, never part of the product.

    python tools/step_ab.py --n 32 --variants "base,sc_side=0" [--steps 50] [--rounds 3]

--samplers ddpm,ddim times the ancestral step and the x0-form step (every timestep a row, so both run the same UNet
evaluations; --eta, --clip-x0) side by side, interleaved like the variants.

--trace times the x0-form step with a score trace attached (the "x0 step + moments" tail and its finalize launch)
against the same build's untraced x0-form step, alternating in one process: arms untraced, traced, untraced again --
the second untraced arm is the A/A spread the difference is read against.

--samplers ddim,dpmpp2m times the second-order step against the x0-form step (--eta is ddim's; dpmpp2m is eta = 0); a
kind may be listed twice (ddim,ddim) for the A/A spread of one step against itself.

--guidance table (--arch c) times the ddim step guided from a constant guidance table (itsd_set_guidance: the x0-form
tail's table-guided instantiation) against the same step guided by the schedule's scalar: arms scalar, table, scalar
again, alternating in one process; the two scalar arms are the A/A spread. --guidance cond-only times the cond-only
step (a table of zeros: the n conditional images alone) against the guided step (a constant table): arms guided,
cond_only, guided again, and the ratio cond_only / guided.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import itsd
from itsd import runtime as rt
from itsd.arch import ARCH_A
from itsd.diffusion import GaussianDiffusionSampler
from itsd.model import UNet


# the shipped value of every option a variant may touch (a variant's keys are reset to these after it runs)
DEFAULTS = {"gn_fold": 1, "p5": 1, "p5_split": 0, "p5_sc": 1, "splitk_inl": 1, "p4_plain": 1, "splitk": 1, "attn_split": 1,
            "p4_sub": 1, "gn_wide": 1, "small_conv": 1, "conv_variant": 2, "small_wide": 1, "small_8x8": 1,
            "subpix_split": 1, "conv1x1": 1, "attn_wide": 1, "attn_wide_nq": 1, "p4_w": 7, "convt_prune": 1, "small_minks": 8,
            "attn_fuse": 1, "fuse_gn": 1, "conv_dbg": 0, "p4_xcd": 2, "spin_bound": 1 << 22, "p4_c96": 1, "p5_dist": 1, "p5_pub": 1, "small_gn": 1, "p5_xl": 3}


def trace_ab(args, smp, x, run_kw):
    """--trace: ms/step of the arms (untraced, traced, untraced again), alternating, args.rounds times."""
    trace = smp.new_trace(args.n)
    arms = [("untraced", None), ("traced", trace), ("untraced_again", None)]
    res = {k: [] for k, _ in arms}
    for r in range(args.rounds):
        for name, tr in arms:
            smp.run(x.clone(), t_begin=999, t_end=999 - 4, seed=1, trace=tr, **run_kw)  # capture + warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp.run(x.clone(), t_begin=999, t_end=999 - args.steps + 1, seed=1, trace=tr, **run_kw)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            res[name].append(ms)
            print(f"round {r} {name}: {ms:.4f} ms/step", flush=True)
    assert bool(torch.isfinite(trace[999 - args.steps + 1:]).all()), "the traced arm left rows unwritten"
    best = {k: min(v) for k, v in res.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    for k in res:
        print(f"{k}: best {best[k]:.4f} median {med[k]:.4f} ms/step")
    base = min(best["untraced"], best["untraced_again"])
    print(f"traced - untraced (best of each): {(best['traced'] - base) * 1e3:+.1f} us/step "
          f"({(best['traced'] / base - 1) * 100:+.3f} %); A/A spread of the two untraced arms: "
          f"{abs(best['untraced'] - best['untraced_again']) * 1e3:.1f} us/step "
          f"({abs(best['untraced'] / best['untraced_again'] - 1) * 100:.3f} %)")


def guidance_ab(args, make, x, run_kw):
    """--guidance: ms/step of three arms, alternating, args.rounds times. Each arm is a sampler of its own on the one
    handle (its warm run installs its schedule and table and captures its graphs before the timed run)."""
    kw = dict(sampler="ddim", steps=1000, eta=args.eta, clip_x0=bool(args.clip_x0))
    const, zeros = torch.full((1000,), 1.8), torch.zeros(1000)
    if args.guidance == "table":
        arms = [("scalar", make(**kw)), ("table", make(guidance=const, **kw)), ("scalar_again", make(**kw))]
    else:
        arms = [("guided", make(guidance=const, **kw)), ("cond_only", make(guidance=zeros, **kw)),
                ("guided_again", make(guidance=const, **kw))]
    res = {k: [] for k, _ in arms}
    for r in range(args.rounds):
        for name, smp in arms:
            smp.run(x.clone(), t_begin=999, t_end=999 - 4, seed=1, **run_kw)  # capture + warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp.run(x.clone(), t_begin=999, t_end=999 - args.steps + 1, seed=1, **run_kw)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            res[name].append(ms)
            want = args.steps if name == "cond_only" else 0
            assert smp.last_cond_only_steps == want, f"{name}: {smp.last_cond_only_steps} cond-only steps"
            print(f"round {r} {name}: {ms:.4f} ms/step", flush=True)
    best = {k: min(v) for k, v in res.items()}
    for k, v in res.items():
        print(f"{k}: best {best[k]:.4f} median {sorted(v)[len(v) // 2]:.4f} ms/step")
    (a, _), (b, _), (a2, _) = arms
    base = min(best[a], best[a2])
    print(f"{b} - {a} (best of each): {(best[b] - base) * 1e3:+.1f} us/step ({(best[b] / base - 1) * 100:+.3f} %), "
          f"ratio {best[b] / base:.4f}; A/A spread of the two {a} arms: {abs(best[a] - best[a2]) * 1e3:.1f} us/step "
          f"({abs(best[a] / best[a2] - 1) * 100:.3f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--img", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", default="base")
    ap.add_argument("--create-set", default="", help="options set before the UNet is created, e.g. attn_fuse=0")
    ap.add_argument("--lib", default="", help="another build of libitsd_hip.so (A/B of two builds in two processes)")
    ap.add_argument("--arch", default="a", help="a: Arch A; c: the C3 leg (Arch C CondUNet, CFG w=1.8: --n is N, 2N guided)")
    ap.add_argument("--samplers", default="ddpm", help="a comma list of ddpm (the ancestral step), ddim (the x0-form step), dpmpp2m (the 2M step); a kind "
                         "listed twice is timed as two arms (A/A)")
    ap.add_argument("--eta", type=float, default=1.0, help="ddim: eta (0: no draw at all)")
    ap.add_argument("--clip-x0", type=int, default=1, help="ddim: clip the x_0 estimate (0 | 1)")
    ap.add_argument("--trace", action="store_true", help="the traced against the untraced ddim step (and an A/A arm)")
    ap.add_argument("--guidance", default="", help="table | cond-only (--arch c): the table-guided / the cond-only ddim "
                                                    "step against the scalar / the guided one (and an A/A arm)")
    args = ap.parse_args()
    if args.guidance:
        if args.guidance not in ("table", "cond-only") or args.arch != "c":
            raise SystemExit("--guidance table | cond-only needs --arch c (a guided model)")
        args.samplers, args.variants = "ddim", "base"
    if args.trace:
        args.samplers, args.variants = "ddim", "base"
    if args.lib:
        rt.LIB_PATH = os.path.abspath(args.lib)
    for kv in filter(None, args.create_set.split("+")):
        k, val = kv.split("=")
        rt.set_option(k, int(val))
    run_kw = {}
    if args.arch == "c":
        from itsd.arch import ARCH_C
        from itsd.diffusion import CondGaussianDiffusionSampler
        from itsd.model import CondUNet
        c = ARCH_C
        net = CondUNet(c.T, c.num_labels, c.ch, c.ch_mult, c.num_res_blocks, 0.0, img_size=args.img, precision="bf16",
                       weights="gauss").to("cuda:0")
        make = lambda **kw: CondGaussianDiffusionSampler(net, 1e-4, 0.028, 1000, w=1.8, **kw)
        run_kw["labels"] = (torch.arange(args.n, device="cuda") % 10 + 1).to(torch.int32)
    else:
        a = ARCH_A
        net = UNet(a.T, a.ch, a.ch_mult, a.attn, a.num_res_blocks, 0.0, img_size=args.img, precision="bf16",
                   weights="gauss").to("cuda:0")
        make = lambda **kw: GaussianDiffusionSampler(net, 1e-4, 0.02, 1000, **kw)
    kinds = args.samplers.split(",")
    kinds = [k if kinds.count(k) == 1 else f"{k}#{kinds[:i].count(k)}" for i, k in enumerate(kinds)]  # ddim#0, ddim#1

    def sampler_of(kind):
        kind = kind.split("#")[0]
        if kind == "ddpm":
            return make()
        if kind == "dpmpp2m":
            return make(sampler="dpmpp2m", steps=1000, clip_x0=bool(args.clip_x0))
        if kind != "ddim":
            raise SystemExit(f"--samplers: unknown kind {kind!r} (ddpm | ddim | dpmpp2m)")
        return make(sampler="ddim", steps=1000, eta=args.eta, clip_x0=bool(args.clip_x0))

    x = torch.randn(args.n, 3, args.img, args.img, device="cuda")
    if args.guidance:
        guidance_ab(args, make, x, run_kw)
        return
    smps = {k: sampler_of(k) for k in kinds}
    variants = [v if len(kinds) == 1 else f"{v}/{k}" for v in args.variants.split(",") for k in kinds]
    if args.trace:
        trace_ab(args, smps["ddim"], x, run_kw)
        return
    res = {v: [] for v in variants}
    for r in range(args.rounds):
        for v in variants:
            smp = smps[v.rsplit("/", 1)[1] if len(kinds) > 1 else kinds[0]]
            v_opts = v.rsplit("/", 1)[0] if len(kinds) > 1 else v
            opts = {}
            for kv in v_opts.split("+"):
                if "=" in kv:
                    k, val = kv.split("=")
                    opts[k] = int(val)
            for k, val in opts.items():
                rt.set_option(k, val)
            smp.run(x.clone(), t_begin=999, t_end=999 - 4, seed=1, **run_kw)  # capture + warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp.run(x.clone(), t_begin=999, t_end=999 - args.steps + 1, seed=1, **run_kw)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            res[v].append(ms)
            for k in opts:  # back to the default of each option touched
                rt.set_option(k, DEFAULTS[k])
            print(f"round {r} {v}: {ms:.4f} ms/step", flush=True)
    for v in variants:
        print(f"{v}: best {min(res[v]):.4f} ms/step  ({args.n * 1000 / min(res[v]) / 1000 * 1000 / 1000:.2f} cand/s at T=1000)")


if __name__ == "__main__":
    main()
