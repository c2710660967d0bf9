"""Latency of max-value entropy search (ABO_ACQ_MES) beside EI, all in the same run, at config 3's shape — N = 8192, d = 8, M = 2^20,
Matérn-5/2 — and at N = 1024, M = 65 536:
  acq       abo_acq_mes against abo_acq with EI, top-100, scores not returned, for S = 16, 64, 256 samples.  MES runs one posterior
            pass and its epilogue; EI at config 3's shape takes the pruned top-k selection, which MES never does — so MES is also set
            beside EI with the scores returned (the full pass).  That difference is the epilogue: reported per (candidate · sample).
  samples   thompson.max_value_samples over the same candidates (S paths in R = 1024 features, their minima).
  optimize  abo_optimize_acquisition_mes beside abo_optimize_acquisition with EI (n_grid = 10 000, n_local = 100), S = 16, over the
            box [−½, 1½]^d: the data fill [0, 1]^d so densely at these N that inside it σ is a few hundredths, γ is in the hundreds, MES
            and EI are flat 0 and no start moves; beyond the data both have something to climb.  A row whose starts took about one
            evaluation each measured the start evaluations only and is marked as such.
There is no bar on these numbers, the file is the record.  Writes mes_latency.txt into --out (default profiles/).

    python tools/mes_latency.py [--iters 5] [--out DIR]
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

SHAPES = [(8192, 1 << 20), (1024, 1 << 16)]
D, K = 8, 100
ELL, SF2, NOISE, XI = 1.0, 1.0, 1e-3, 0.01
SAMPLES = (16, 64, 256)


def timed(fn, iters, model):
    import torch
    wall, dev = [], []
    out = None
    for r in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r:
            wall.append((time.perf_counter() - t0) * 1e3); dev.append(model.timings()["acq_total_ms"])
    return float(np.median(wall)), float(np.median(dev)), out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    lines = [f"MES beside EI, d={D} Matern-5/2 ell={ELL} noise={NOISE}; median of {a.iters} calls after one warm-up"]
    for N, M in SHAPES:
        X, y = synth.standardized_problem(N, D, float(np.sqrt(NOISE)))
        Z = torch.from_numpy(synth.points(2, M, D)).cuda()
        model = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE, device=0), X, y)
        best = float(y.min())
        ei = abo.ExpectedImprovement(XI, best)
        lines += [f"N={N}, top-{K} of M={M} device-resident candidates:",
                  f"{'objective':>22} {'wall ms':>9} {'device ms':>10} {'pruned':>7} {'ns per (candidate·sample) over EI full':>39}"]
        w, dv, _ = timed(lambda: abo.evaluate(ei, model, Z, k=K, return_scores=False), a.iters, model)
        lines.append(f"{'EI, top-k only':>22} {w:9.3f} {dv:10.3f} {model.prune_stats()['pruned']:7d}")
        w, dv_full, _ = timed(lambda: abo.evaluate(ei, model, Z, k=K, return_scores=True), a.iters, model)
        lines.append(f"{'EI, scores returned':>22} {w:9.3f} {dv_full:10.3f} {model.prune_stats()['pruned']:7d}")
        draws = {}
        for S in SAMPLES:
            abo.max_value_samples(model, Z, S, R=1024, rng=S)                 # (warm-up: the first call allocates)
            t0 = time.perf_counter()
            ys = abo.max_value_samples(model, Z, S, R=1024, rng=S + 1)
            draws[S] = ((time.perf_counter() - t0) * 1e3, ys)
            acq = abo.MaxValueEntropySearch(ys)
            w, dv, out = timed(lambda: abo.evaluate(acq, model, Z, k=K, return_scores=False), a.iters, model)
            per = (dv - dv_full) * 1e6 / (M * S)
            lines.append(f"{f'MES, S = {S}':>22} {w:9.3f} {dv:10.3f} {model.prune_stats()['pruned']:7d} {per:39.4f}")
        lines.append("max_value_samples over the same candidates (R = 1024; wall ms, host draws and the copy of the base arrays included):")
        for S in SAMPLES:
            lines.append(f"{f'S = {S}':>22} {draws[S][0]:9.3f}   y* {draws[S][1].min():.3f} … {draws[S][1].max():.3f} (min y {best:.3f})")
        dom = abo.ContinuousDomain(np.full(D, -0.5), np.full(D, 1.5))
        lines += ["optimize_acquisition over [-0.5, 1.5]^d, n_grid = 10000, n_local = 100:",
                  f"{'objective':>22} {'wall ms':>9} {'refine ms':>10} {'evals/start':>12} {'median gain over the start':>27}"]
        for name, acq in (("EI", ei), ("MES, S = 16", abo.MaxValueEntropySearch(draws[16][1]))):
            wall, ref, evals = [], [], []
            for r in range(a.iters + 1):
                t0 = time.perf_counter()
                _, _, sx, sv, rx, rv = abo.optimize_acquisition_device(acq, model, dom, 10_000, 100, seed=r, return_all=True)
                if r:
                    t = model.timings()
                    wall.append((time.perf_counter() - t0) * 1e3); ref.append(t["refine_ms"])
                    evals.append(t["refine_evals"] / max(t["refine_starts"], 1))
            flat = "   (no start moved: the start evaluations only)" if np.median(evals) < 1.5 else ""
            lines.append(f"{name:>22} {np.median(wall):9.3f} {np.median(ref):10.3f} {np.median(evals):12.2f} {np.median(rv - sv):27.3e}{flat}")
    txt = "\n".join(lines)
    print(txt)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "mes_latency.txt"), "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
