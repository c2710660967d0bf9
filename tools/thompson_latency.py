"""Latency of Thompson sampling by pathwise sample paths (abo_paths_create / abo_paths_eval, top-1 only) at the shapes of configs
2, 3 and 5 (one device), for S in {16, 64} paths and R in {1024, 4096} features, beside
  * the same model's abo_acq EI call on the same candidates in the same process (what a user would run instead), and
  * a yardstick for the pass: max(2·(N + R)·M·S / fp64 MFMA peak, time of a μ-only abo_predict on the same Z) — the generated operand
    costs the N·M kernel evaluations the μ pass does anyway.  The μ pass is a measured time of another kernel, not a lower bound:
    the ratio "yard/eval" can exceed 1.
A one-shot Thompson batch pays create + eval: that sum stands beside EI ("EI/(c+e)").
Times are the library's HIP-event times (abo_paths_stats_get, abo_get_timings), every column the median of --iters calls after one
warm-up (create: --iters + 1 objects made from the same base arrays).
Writes thompson_latency.{json,txt} into --out (default profiles/).

    python tools/thompson_latency.py [--iters 3] [--configs c2,c3,c5] [--out DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abstractbayesopt.jl_amd as abo  # noqa: E402
from abstractbayesopt.jl_amd import synth  # noqa: E402

PEAK_FP64_MFMA = 78.6e12
#          kernel                       d   N      M        ell  sf2  noise
SHAPES = {"c2": (abo.SqExponentialKernel, 4, 1024, 65536, 0.5, 1.0, 1e-4),
          "c3": (abo.Matern52Kernel, 8, 8192, 1 << 20, 1.0, 1.0, 1e-3),
          "c5": (abo.Matern52Kernel, 16, 16384, 131072, 2.0, 1.0, 1e-2)}


def median_of(f, iters):
    f()
    return float(np.median([f() for _ in range(iters)]))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        kern, d, N, M, ell, sf2, noise = SHAPES[name]
        X = synth.points(1, N, d)
        y = synth.objective(X, 0.05)
        Z = torch.from_numpy(synth.points(2, M, d)).cuda()
        model = abo.update(abo.HipStandardGP(sf2 * abo.with_lengthscale(kern(), ell), noise, device=0), X, y)
        ei = abo.ExpectedImprovement(0.01, float(y.min()))

        def ei_ms():
            abo.evaluate(ei, model, Z, k=1, return_scores=False)
            return model.timings()["acq_total_ms"]

        def mu_ms():
            abo.posterior_mean(model, Z)
            return model.timings()["acq_total_ms"]

        t_ei, t_mu = median_of(ei_ms, a.iters), median_of(mu_ms, a.iters)
        for S in (16, 64):
            for R in (1024, 4096):
                paths = abo.sample_paths(model, S, R, rng=1)
                base = (paths.omega, paths.phase, paths.w, paths.eps)
                create = median_of(lambda: abo.SamplePaths(model, *base).stats()["create_ms"], a.iters)

                def ev_ms():
                    paths.argmin(Z, k=1)
                    return paths.stats()["eval_ms"]

                t = median_of(ev_ms, a.iters)
                flop = paths.stats()["eval_flop"]
                bound = max(flop / PEAK_FP64_MFMA * 1e3, t_mu)
                rows.append({"config": name, "N": N, "d": d, "M": M, "S": S, "R": R, "create_ms": create, "eval_top1_ms": t,
                             "eval_flop": flop, "eval_tflops": flop / t / 1e9, "ei_acq_ms": t_ei, "mu_predict_ms": t_mu,
                             "yardstick_ms": bound, "yardstick_over_eval": bound / t, "ei_over_eval": t_ei / t,
                             "ei_over_create_plus_eval": t_ei / (create + t)})
                del paths
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "thompson_latency.json"), "w") as f:
        json.dump({"unit": "ms (HIP events)", "iters": a.iters, "fp64_mfma_peak_flops": PEAK_FP64_MFMA, "rows": rows}, f, indent=1)
    lines = ["Thompson sampling by sample paths, top-1 per path (HIP-event ms, median of %d); yard = max(MFMA time at 78.6 TFLOP/s, mu-only predict); c+e = create + eval" % a.iters,
             "%4s %6s %8s %4s %5s %10s %10s %8s %10s %10s %9s %9s %8s %9s" % ("cfg", "N", "M", "S", "R", "create", "eval", "TFLOP/s", "EI acq",
                                                                      "mu only", "yard", "yard/eval", "EI/eval", "EI/(c+e)")]
    for r in rows:
        lines.append("%4s %6d %8d %4d %5d %10.3f %10.3f %8.2f %10.3f %10.3f %9.3f %9.2f %8.1f %9.1f" % (
            r["config"], r["N"], r["M"], r["S"], r["R"], r["create_ms"], r["eval_top1_ms"], r["eval_tflops"], r["ei_acq_ms"],
            r["mu_predict_ms"], r["yardstick_ms"], r["yardstick_over_eval"], r["ei_over_eval"], r["ei_over_create_plus_eval"]))
    with open(os.path.join(a.out, "thompson_latency.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
