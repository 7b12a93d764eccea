"""Hash of what the sampler tail writes, in each of its modes, for a build given by --lib: bit-identity checks between
two builds run as two processes (tools/fwd_hash.py is the same for the forward alone). Measurement tool, never part of
the product.

    python tools/tail_hash.py [--lib path/to/libitsd_hip.so]

One line per tail form of TAIL_CASES (tests/test_gpu_path_branch.py: every tail kernel, bf16 and fp32, plain and
guided), fixed seeds, sha256 of: the forward's eps, one ancestral step, predict_x0, a 6-row ddim run with eta = 1, the
same run traced and its trace, one verify_denoise sse.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch


def _h(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    from itsd import runtime as rt
    if args.lib:
        rt.LIB_PATH = os.path.abspath(args.lib)
    from itsd.diffusion import CondGaussianDiffusionSampler, GaussianDiffusionSampler
    from test_gpu_path_branch import DEV, TAIL_CASES, T, _net, _x

    for case, (a, precision, io_mfma, n) in TAIL_CASES.items():
        rt.set_option("io_mfma", io_mfma)  # (read when the native handle is created: every first call is in here)
        try:
            net = _net(a, precision)
            kind, kw = (CondGaussianDiffusionSampler, {"w": 1.8}) if a.cfg else (GaussianDiffusionSampler, {})
            beta_T = 0.028 if a.cfg else 0.02
            ddpm = kind(net, 1e-4, beta_T, T, **kw)
            ddim = kind(net, 1e-4, beta_T, T, sampler="ddim", steps=6, eta=1.0, clip_x0=True, **kw)
            x = _x(n, a.img_size, seed=3)
            lab = torch.tensor([3, 7, 1], dtype=torch.int32, device=DEV)[:n] if a.cfg else None
            out = {"eps": (net(x, 5, lab) if a.cfg else net(x, 5)).float()}
            out["step"] = ddpm.run(x.clone(), t_begin=5, t_end=5, labels=lab, seed=7, clip=False)
            out["x0"] = ddpm.predict_x0(x, 5, labels=lab)
            out["ddim"] = ddim.run(x.clone(), labels=lab, seed=7)
            trace = ddim.new_trace(n)
            out["traced"] = ddim.run(x.clone(), labels=lab, seed=7, trace=trace)
            out["trace"] = trace
            sse = torch.full((n, 2), float("nan"), dtype=torch.float64, device=DEV)
            ddpm._native(n).verify_denoise(x, 5, 0.8, 0.6, 0x5EED, 0xD0000001, labels=lab, sse=sse)
            out["sse"] = sse
            torch.cuda.synchronize()
        finally:
            rt.set_option("io_mfma", 1)
        print(f"{case}: " + " ".join(f"{k}={_h(v)}" for k, v in out.items()), flush=True)


if __name__ == "__main__":
    main()
