"""Latency of a Thompson step on sample paths that FOLLOW the model (abo_append → abo_cand_downdate → abo_paths_append →
abo_paths_top, k = 1) at config 5's shape (N = 16 384, d = 16, M = 131 072) and at N = 8 192, d = 8, M = 2²⁰, for S in {16, 64} paths in
R = 1024 features — and, in the SAME run on the same model and resident set, what the step costs without it: abo_paths_create +
abo_paths_eval_cand(k = 1) on the appended model (those two entry points are what a step had to call before abo_paths_append existed).
Times are the library's HIP-event times (abo_paths_append_stats_get, abo_paths_stats_get); abo_paths_top is host wall clock (its
k = 1 form launches one tiny kernel).  Every column is the median of --iters real appends after one warm-up append.  The resident
update's rate = (16·S·M + 8·M) bytes / its time, beside the 8 TB/s HBM peak and the 6.4 TB/s cand_gemv_kernel reaches (DESIGN K7).
Writes thompson_append_latency.{json,txt} into --out (default profiles/).

    python tools/thompson_append_latency.py [--iters 5] [--configs c5,n8k] [--out DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abstractbayesopt.jl_amd as abo  # noqa: E402
from abstractbayesopt.jl_amd import synth  # noqa: E402

HBM_PEAK, STREAM_YARD = 8.0e12, 6.4e12
#          kernel               d   N      M         ell  sf2  noise
SHAPES = {"c5": (abo.Matern52Kernel, 16, 16384, 131072, 2.0, 1.0, 1e-2),
          "n8k": (abo.Matern52Kernel, 8, 8192, 1 << 20, 1.0, 1.0, 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--configs", default="c5,n8k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        kern, d, N, M, ell, sf2, noise = SHAPES[name]
        steps = a.iters + 1
        X = synth.points(1, N + 2 * steps, d)
        y = synth.objective(X, 0.05)
        Z = synth.points(2, M, d)
        for S in (16, 64):
            model = abo.update(abo.HipStandardGP(sf2 * abo.with_lengthscale(kern(), ell), noise, device=0, n_max=N + 4 * steps), X[:N], y[:N])
            cands = abo.ResidentCandidates(model, Z)
            paths = abo.sample_paths(model, S, 1024, rng=1)
            paths.attach(cands)
            rng = np.random.default_rng(2)
            cols = {k: [] for k in ("model_ms", "resident_ms", "top_ms", "create_ms", "eval_ms", "downdate_ms")}
            m = model
            for j in range(steps):
                m = abo.append(m, X[N + j], float(y[N + j]))
                cands.downdate(m)
                cols["downdate_ms"].append(m.timings()["downdate_ms"])
                paths.append(m, rng=rng)
                st = paths.append_stats()
                t0 = time.perf_counter()
                paths.top(1)
                cols["top_ms"].append((time.perf_counter() - t0) * 1e3)
                cols["model_ms"].append(st["model_ms"])
                cols["resident_ms"].append(st["resident_ms"])
                # the same step without abo_paths_append: new paths on the appended model, evaluated over the set
                fresh = abo.SamplePaths(m, paths.omega, paths.phase, paths.w, paths.eps)
                fresh.argmin(cands, k=1)
                fs = fresh.stats()
                cols["create_ms"].append(fs["create_ms"])
                cols["eval_ms"].append(fs["eval_ms"])
                del fresh
            med = {k: float(np.median(v[1:])) for k, v in cols.items()}
            nbytes = st["resident_bytes"]
            rate = nbytes / (med["resident_ms"] * 1e-3)
            step_new = med["model_ms"] + med["resident_ms"] + med["top_ms"]
            step_old = med["create_ms"] + med["eval_ms"]
            rows.append(dict(config=name, N=N, d=d, M=M, S=S, R=1024, **med, resident_bytes=nbytes, resident_TBps=rate / 1e12,
                             of_hbm_peak=rate / HBM_PEAK, of_stream_yardstick=rate / STREAM_YARD, column_from_chain=st["column_from_chain"],
                             step_append_ms=step_new, step_create_eval_ms=step_old, ratio=step_old / step_new))
            paths.detach()
            del paths, cands, model, m
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "thompson_append_latency.json"), "w") as f:
        json.dump({"unit": "ms (HIP events; top: host wall clock)", "iters": a.iters, "hbm_peak": HBM_PEAK, "stream_yardstick": STREAM_YARD,
                   "rows": rows}, f, indent=1)
    lines = ["Thompson step on paths that follow the model (median of %d real appends after one warm-up; ms).  append = abo_paths_append "
             "(model: g_s(x*) + V update; resident: rank-1 update of S x M values + fused arg-min), top = abo_paths_top(k=1); "
             "create + eval = the same step by abo_paths_create + abo_paths_eval_cand(k=1), same run, same model and set" % a.iters,
             "%4s %6s %8s %4s %9s %9s %9s %8s %7s %7s %10s %10s %10s %7s" % ("cfg", "N", "M", "S", "model", "resident", "top", "TB/s", "/8.0", "/6.4",
                                                                         "create", "eval", "downdate", "ratio")]
    for r in rows:
        lines.append("%4s %6d %8d %4d %9.4f %9.4f %9.4f %8.2f %7.2f %7.2f %10.3f %10.3f %10.4f %7.1f" % (
            r["config"], r["N"], r["M"], r["S"], r["model_ms"], r["resident_ms"], r["top_ms"], r["resident_TBps"], r["of_hbm_peak"],
            r["of_stream_yardstick"], r["create_ms"], r["eval_ms"], r["downdate_ms"], r["ratio"]))
    with open(os.path.join(a.out, "thompson_append_latency.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
