"""Latency of LogEI (ABO_ACQ_LOGEI) beside EI, both in the same run:
  top-k    abo_acq, k = 100, scores not returned (the pruned top-k selection where it is eligible), at config 3's shape — N = 8192, d = 8,
           M = 2^20, Matérn-5/2, ξ = 0.01 — with the survivor counts of abo_get_prune_stats;
  optimize abo_optimize_acquisition (n_grid = 10 000, n_local = 100) at N = 8192, d = 8, with ξ = 0.01 and with a ξ at which EI has
           left the range its stopping rules can see; accepted iterations are not kept per start by the one-call entry, so the figure
           reported is abo_timings.refine_evals / refine_starts: objective evaluations (value + gradient) per start, 1 = the start only.
The epilogue is O(M) under an N²·M contraction: there is no bar on these numbers, the file is the record.
Writes logei_latency.txt into --out (default profiles/).

    python tools/logei_latency.py [--iters 5] [--out DIR]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abstractbayesopt.jl_amd as abo  # noqa: E402
from abstractbayesopt.jl_amd import synth  # noqa: E402

N, D, M, K = 8192, 8, 1 << 20, 100
ELL, SF2, NOISE, XI = 1.0, 1.0, 1e-3, 0.01


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    X, y = synth.standardized_problem(N, D, float(np.sqrt(NOISE)))
    Z = torch.from_numpy(synth.points(2, M, D)).cuda()
    model = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE, device=0), X, y)
    best = float(y.min())
    lines = [f"LogEI beside EI, N={N} d={D} Matern-5/2 ell={ELL} noise={NOISE}; median of {a.iters} calls after one warm-up",
             f"top-{K} of M={M} device-resident candidates (abo_acq, scores not returned):",
             f"{'kind':>6} {'xi':>8} {'wall ms':>9} {'device ms':>10} {'pruned':>7} {'survivors':>10} {'finite':>7} {'distinct':>9}"]
    far = None
    for xi in (XI, None):
        if xi is None:                       # a ξ that puts every candidate at z ≤ −40: EI is 0.0 on the whole grid
            mu, var = abo.mean_and_var(model, Z[:65536])
            mu, var = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (mu, var))
            xi = far = float(np.max(best - mu + 45.0 * np.sqrt(var)))
        for name, acq in (("EI", abo.ExpectedImprovement(xi, best)), ("LOGEI", abo.LogExpectedImprovement(xi, best))):
            wall, dev = [], []
            for r in range(a.iters + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
                torch.cuda.synchronize()
                if r:
                    wall.append((time.perf_counter() - t0) * 1e3); dev.append(model.timings()["acq_total_ms"])
            st = model.prune_stats()
            tv = tv.cpu().numpy()
            lines.append(f"{name:>6} {xi:8.3f} {np.median(wall):9.3f} {np.median(dev):10.3f} {st['pruned']:7d} {st['survivors']:10d} "
                         f"{int(np.sum(np.isfinite(tv))):7d} {len(np.unique(tv)):9d}")
    dom = abo.ContinuousDomain(np.zeros(D), np.ones(D))
    lines += ["abo_optimize_acquisition, n_grid = 10000, n_local = 100:",
              f"{'kind':>6} {'xi':>8} {'wall ms':>9} {'refine ms':>10} {'evals/start':>12} {'median gain over the start':>27}"]
    for xi in (XI, far):
        for name, acq in (("EI", abo.ExpectedImprovement(xi, best)), ("LOGEI", abo.LogExpectedImprovement(xi, best))):
            wall, ref, evals = [], [], []
            for r in range(a.iters + 1):
                t0 = time.perf_counter()
                _, _, sx, sv, rx, rv = abo.optimize_acquisition_device(acq, model, dom, 10_000, 100, seed=r, return_all=True)
                if r:
                    t = model.timings()
                    wall.append((time.perf_counter() - t0) * 1e3); ref.append(t["refine_ms"])
                    evals.append(t["refine_evals"] / max(t["refine_starts"], 1))
            lines.append(f"{name:>6} {xi:8.3f} {np.median(wall):9.3f} {np.median(ref):10.3f} {np.median(evals):12.2f} {np.median(rv - sv):27.3e}")
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "logei_latency.txt"), "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
