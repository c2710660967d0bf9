"""Latency of append_points(model, xs, ys) (abo_append_batch: k observations in one blocked bordered step) beside what exists without
it, measured in ONE process, alternating per repetition:
  * abo_append_batch on k points,
  * k sequential abo_append of the same points (the yardstick: the code path abo_update's appends take),
  * one refit of the N + k points,
for N = 1024, 8192, 16384 and k = 1, 2, 3, 4, 8, 16, 32, 64; d = 8, Matern-5/2.  Host time per call in ms, median [p10, p90], and the device
time of the two block products (abo_timings.append_trmv_ms) beside the one-append mat-vec pair of the same run.

    python tools/append_batch_latency.py [--reps 9] [--out profiles/append_batch_latency.txt]
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

D, ELL, SF2, NOISE = 8, 1.0, 1.0, 1e-2
KS = (1, 2, 3, 4, 8, 16, 32, 64)


def model(n_max):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE, device=0, n_max=n_max)


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.asarray(v)
    return float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))


def sweep(N, reps, refit_reps):
    X = synth.points(12, N + max(KS), D)
    y = synth.objective(X, 0.05)
    plain = model(0)
    base = abo.update(model(N + max(KS) + 128), X[:N], y[:N])
    rows = []
    for k in KS:
        xb, yb = np.ascontiguousarray(X[N:N + k]), np.ascontiguousarray(y[N:N + k])
        tb, ts, tr, dev_b, dev_1 = [], [], [], [], []
        for r in range(reps + 1):
            m, t_b = ms(lambda: abo.append_points(base, xb, yb))
            assert m.append_path == "appended"
            trmv_b = m.timings()["append_trmv_ms"]
            del m                                     # its rows go back: the chain below appends in place

            def chain():
                c = base
                for j in range(k):
                    c = abo.append(c, X[N + j], y[N + j])
                return c
            c, t_s = ms(chain)
            del c
            one = abo.append(base, X[N], y[N])
            trmv_1 = one.timings()["append_trmv_ms"]
            del one
            t_r = None
            if r <= refit_reps:
                _, t_r = ms(lambda: abo.update(plain, X[:N + k], y[:N + k]))
            if r:
                tb.append(t_b); ts.append(t_s); dev_b.append(trmv_b); dev_1.append(trmv_1)
                if t_r is not None:
                    tr.append(t_r)
        rows.append({"k": k, "batch": stats(tb), "seq": stats(ts), "refit": stats(tr), "dev_batch": stats(dev_b), "dev_one": stats(dev_1)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--refit-reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 8192, 16384])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_batch_latency.txt"))
    a = ap.parse_args()
    f = lambda s: f"{s[0]:8.3f} [{s[1]:.3f}, {s[2]:.3f}]"
    lines = [f"append_points(model, xs, ys) (abo_append_batch) vs k sequential abo_append vs one refit of N + k points, d = {D}, Matern-5/2, "
             f"alternated in one process; ms per call, median [p10, p90] of {a.reps} (refit: of {a.refit_reps}); "
             "products = device time of the two block products of the batch (HIP events), mat-vecs = of ONE append's two mat-vecs"]
    for N in a.sizes:
        for r in sweep(N, a.reps, a.refit_reps):
            below = "yes" if r["batch"][0] < r["seq"][1] else "NO"
            lines.append(f"N={N:6d} k={r['k']:3d}  batch {f(r['batch'])}  sequential {f(r['seq'])}  refit {f(r['refit'])}  "
                         f"batch/sequential {r['batch'][0] / r['seq'][0]:.3f}  batch/refit {r['batch'][0] / r['refit'][0]:.3f}  "
                         f"batch median < sequential p10: {below}  products {f(r['dev_batch'])}  mat-vecs {f(r['dev_one'])}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
