"""Latency of remove_points(model, idx) (abo_remove: one observation out of the factor in O(N²)) against the refit of the remaining
points (abo_create + abo_fit from host arrays, what update(model, xs, ys) does), alternated in one process, d = 8, Matérn-5/2:
  * one removal at j = 0 (the whole trailing block changes: the worst case), j = N/2 and j = N − 1 (copies only), N = 1024, 8192, 16384;
  * a k sweep — k single removals, highest index first, against one refit of the N − k remaining points — at N = 1024 and 8192:
    what the crossover rule of abo_remove (include/abo_hip.h) is set from;
  * one sliding-window step: remove the oldest point and append a new one, against the refit of the new window.
Writes remove_latency.{json,txt} into --out (default profiles/).

    python tools/remove_latency.py [--iters 30] [--warmup 3] [--sizes 1024,8192,16384] [--out DIR]
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

D, ELL, SF2, NOISE = 8, 1.0, 1.0, 1e-2


def model(n_max=0):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE, device=0, n_max=n_max)


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "n": int(v.size)}


def fmt(s):
    return f"{s['median']:.3f} [{s['p10']:.3f}, {s['p90']:.3f}]"


def single(N, iters, warmup):
    X = synth.points(11, N + 1, D)
    y = synth.objective(X, 0.05)
    plain = model()
    base = abo.update(model(N), X[:N], y[:N])
    out = {}
    for name, j in (("j=0", 0), ("j=N/2", N // 2), ("j=N-1", N - 1)):
        keep = np.r_[0:j, j + 1:N]
        Xk, yk = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])
        tr, tf = [], []
        for it in range(warmup + iters):
            m, t = ms(lambda: abo.remove_points(base, j))
            assert m.remove_path == "removed"
            del m
            r, t2 = ms(lambda: abo.update(plain, Xk, yk))
            del r
            if it >= warmup:
                tr.append(t); tf.append(t2)
        out[name] = {"remove": stats(tr), "refit": stats(tf), "speedup_median": float(np.median(tf) / np.median(tr))}
    # sliding window: the oldest point out, a new one in
    Xw, yw = np.ascontiguousarray(X[1:N + 1]), np.ascontiguousarray(y[1:N + 1])
    tw, tf = [], []
    for it in range(warmup + iters):
        def step():
            return abo.append(abo.remove_points(base, 0), X[N], y[N])
        m, t = ms(step)
        del m
        r, t2 = ms(lambda: abo.update(plain, Xw, yw))
        del r
        if it >= warmup:
            tw.append(t); tf.append(t2)
    out["window"] = {"step": stats(tw), "refit": stats(tf), "speedup_median": float(np.median(tf) / np.median(tw))}
    return out


def sweep(N, ks, reps):
    X = synth.points(12, N, D)
    y = synth.objective(X, 0.05)
    plain = model()
    base = abo.update(model(N), X, y)
    rows = []
    for k in ks:
        idx = np.linspace(0, N - 1, k).astype(np.int64) if k > 1 else np.array([0], dtype=np.int64)      # spread over the factor, 0 included
        idx = np.unique(idx)
        keep = np.setdiff1d(np.arange(N), idx)
        Xk, yk = np.ascontiguousarray(X[keep]), np.ascontiguousarray(y[keep])
        ta, tr = [], []
        for r in range(reps + 1):
            def chain():
                m = base
                for j in idx[::-1]:
                    m = abo.remove_points(m, int(j))
                return m
            m, t = ms(chain)
            del m
            f, t2 = ms(lambda: abo.update(plain, Xk, yk))
            del f
            if r:
                ta.append(t); tr.append(t2)
        rows.append({"k": int(len(idx)), "removals_ms": float(np.median(ta)), "refit_ms": float(np.median(tr)),
                     "ratio": float(np.median(ta) / np.median(tr))})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1024,8192,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of the record")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = {"d": D, "kernel": "Matern52", "noise": NOISE, "device": torch.cuda.get_device_name(0), "single": {}, "k_sweep": {}}
    lines = [f"remove_points(model, idx) (abo_remove) vs the refit of the remaining points, d = {D}, Matern-5/2, {a.iters} iterations "
             f"after {a.warmup} warm-up, alternated in one process; ms per call (median [p10, p90])"]
    for N in [int(s) for s in a.sizes.split(",")]:
        r = single(N, a.iters, a.warmup)
        res["single"][str(N)] = r
        for name in ("j=0", "j=N/2", "j=N-1"):
            lines.append(f"N={N:6d} {name:6s}  remove {fmt(r[name]['remove'])}  refit {fmt(r[name]['refit'])}  "
                         f"speed-up {r[name]['speedup_median']:.1f}x")
            print(lines[-1]); sys.stdout.flush()
        w = r["window"]
        lines.append(f"N={N:6d} window  remove oldest + append {fmt(w['step'])}  refit {fmt(w['refit'])}  speed-up {w['speedup_median']:.1f}x")
        print(lines[-1]); sys.stdout.flush()
    ks = [1, 2, 4, 8, 16, 32, 64]
    lines.append(f"k sweep: k single removals (indices spread over the factor, highest first) vs one refit of the N - k remaining points "
                 f"(ms, median of {a.reps}); ratio < 1: removing is cheaper")
    for N in (1024, 8192):
        rows = sweep(N, ks, a.reps)
        res["k_sweep"][str(N)] = rows
        for row in rows:
            lines.append(f"N={N:6d} k={row['k']:3d}  removals {row['removals_ms']:8.3f}  refit {row['refit_ms']:8.3f}  ratio {row['ratio']:.3f}")
            print(lines[-1]); sys.stdout.flush()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "remove_latency.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(a.out, "remove_latency.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
