#!/usr/bin/env python
"""Time the Matern signature kernels (the radial seed) beside SignatureRBF and SignatureLinear of the same build.

  K(X) normalised, N = 1024, D = 5, M = 5, L = 100 and 128: SignatureMatern12 / 32 / 52, SignatureRBF (the
  hand-tuned packed seed) and SignatureLinear (the generic per-row seed with one dot per cell).

Per kernel and length: the whole K(X) call (diagonal launch + Gram launch) and the raw Gram launch alone, each
as the median of --steps HIP-event timings after --warmup calls, inputs resident; then the ratios to RBF and
to linear.  One JSON object per row to stdout and to --out.

    python tools/bench_matern.py --out profiles/matern_rows.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walks(n, l, d, seed):
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.standard_normal((n, l, d)), axis=1) / np.sqrt(l * d)).astype(np.float32)


def event_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--d", type=int, default=5)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--lengths", type=int, nargs="+", default=[100, 128])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import gpsig_amd
    from gpsig_amd import ops

    dev = torch.device("cuda", 0)
    kernels = [("rbf", gpsig_amd.SignatureRBF), ("linear", gpsig_amd.SignatureLinear),
               ("matern12", gpsig_amd.SignatureMatern12), ("matern32", gpsig_amd.SignatureMatern32),
               ("matern52", gpsig_amd.SignatureMatern52)]
    rows = []
    for l in args.lengths:
        X = torch.as_tensor(walks(args.n, l, args.d, 0).reshape(args.n, -1), device=dev)
        res = {}
        for base, cls in kernels:
            k = cls(l * args.d, args.d, args.levels).to(dev)
            Xs = k._prep(X)
            res[base] = dict(K_ms=event_ms(lambda: k.K(X), args.steps, args.warmup),
                             gram_ms=event_ms(lambda: ops.sig_gram(Xs, None, args.levels, base=base), args.steps,
                                              args.warmup))
        for base, _ in kernels:
            r = res[base]
            rows.append(dict(workload=f"K(X) normalised N={args.n} L={l} D={args.d} M={args.levels}", base=base,
                             K_ms=round(r["K_ms"], 3), gram_ms=round(r["gram_ms"], 3),
                             gram_vs_rbf=round(r["gram_ms"] / res["rbf"]["gram_ms"], 2),
                             gram_vs_linear=round(r["gram_ms"] / res["linear"]["gram_ms"], 2),
                             steps=args.steps, warmup=args.warmup))
    text = "\n".join(json.dumps(r) for r in rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
