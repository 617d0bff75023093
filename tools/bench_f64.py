#!/usr/bin/env python
"""Time the float64 evaluation path (precision="float64") beside the float32 kernels of the same build.

  K(X) normalised, N = 1024, D = 5, M = 5, L = 100 and 128: SignatureRBF, SignatureLinear, SignatureMatern32.

Per kernel and length: the whole K(X) call (diagonal launch + Gram launch) and the raw Gram launch alone, in
float64 and in float32 in the same run, each as the median of --steps HIP-event timings after --warmup calls,
inputs resident; their ratios; and max|K64 - K32| / max|K64| of the normalised K on that data.  One JSON object
per row to stdout and to --out.

    python tools/bench_f64.py --out profiles/f64_rows.jsonl
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
               ("matern32", gpsig_amd.SignatureMatern32)]
    rows = []
    for l in args.lengths:
        X32 = torch.as_tensor(walks(args.n, l, args.d, 0).reshape(args.n, -1), device=dev)
        X64 = X32.double()
        for base, cls in kernels:
            k32 = cls(l * args.d, args.d, args.levels).to(dev)
            k64 = cls(l * args.d, args.d, args.levels, precision="float64").to(dev)
            Xs32, Xs64 = k32._prep(X32), k64._prep(X64)
            K64, K32 = k64.K(X64), k32.K(X32)
            diff = float((K64 - K32.double()).abs().max() / K64.abs().max())
            t = dict(K64_ms=event_ms(lambda: k64.K(X64), args.steps, args.warmup),
                     K32_ms=event_ms(lambda: k32.K(X32), args.steps, args.warmup),
                     gram64_ms=event_ms(lambda: ops.sig_gram_f64(Xs64, None, args.levels, base=base), args.steps,
                                        args.warmup),
                     gram32_ms=event_ms(lambda: ops.sig_gram(Xs32, None, args.levels, base=base), args.steps,
                                        args.warmup))
            rows.append(dict(workload=f"K(X) normalised N={args.n} L={l} D={args.d} M={args.levels}", base=base,
                             route=ops.f64_route(l, None, args.levels),
                             **{n: round(v, 3) for n, v in t.items()},
                             K_f64_over_f32=round(t["K64_ms"] / t["K32_ms"], 2),
                             gram_f64_over_f32=round(t["gram64_ms"] / t["gram32_ms"], 2),
                             max_abs_K64_minus_K32_over_max_K64=diff, steps=args.steps, warmup=args.warmup))
    text = "\n".join(json.dumps(r) for r in rows)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
