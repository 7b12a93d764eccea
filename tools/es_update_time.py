"""Wall time of one update of the gradient search: itsd_es_candidates (the next round's 2M candidates) + itsd_es_step
(the gradient's slice sums, the Adam step, the norm), timed with device events, warm, the median of `--reps` runs, at
(M pairs, per elements) points. For DESIGN.md section 12; the product never imports this.

    python tools/es_update_time.py [--points 128x3072,512x49152] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from itsd import runtime as rt  # noqa: E402
from itsd.schedule import adam_coeffs  # noqa: E402


def _ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def point(n_pairs, per, reps, dev):
    theta = torch.randn(per, device=dev)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    w = torch.randn(n_pairs, device=dev) * 1e-3
    ws = torch.empty(rt.es_workspace_bytes(n_pairs, per), dtype=torch.uint8, device=dev)
    out = torch.empty(2 * n_pairs, per, device=dev)
    gn2 = torch.zeros(1, dtype=torch.float64, device=dev)
    adam = adam_coeffs(0.01, (0.9, 0.999), 1e-8, 5)

    def cands():
        rt.es_candidates(out, theta, 2 * n_pairs, 0.05, 7, 0xB0000001)

    def step():
        rt.es_step(theta, m, v, w, 7, 0xB0000001, adam, ws, gnorm2=gn2)

    def both():
        cands()
        step()

    for _ in range(3):  # warm: code objects loaded, buffers touched
        both()
    torch.cuda.synchronize()
    r = {"n_pairs": n_pairs, "per": per, "candidates": 2 * n_pairs, "reps": reps,
         "candidate_bytes": out.numel() * 4, "workspace_bytes": ws.numel()}
    for name, fn in (("update_ms", both), ("es_candidates_ms", cands), ("es_step_ms", step)):
        med, lo, hi = _ms(fn, reps)
        r[name] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="128x3072,512x49152")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("es_update_time.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    rows = []
    for p in args.points.split(","):
        m, per = (int(x) for x in p.split("x"))
        rows.append(point(m, per, args.reps, dev))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "points": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
