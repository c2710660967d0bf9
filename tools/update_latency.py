"""Latency of update(model, xs, ys) in a driver-shaped loop (one fit, then one new point per iteration, src/bayesian_opt.jl:119-125):
the refit path (incremental_update=False: abo_create + abo_fit) against the incremental path (abo_update: prefix match + bordered
append), alternated in one process, d = 8, Matérn-5/2, at N0 = 1024, 8192, 16384.  The incremental call is split into
  match   — abo_update on the SAME data (k = 0): host → device staging, the prefix-match kernel, the one read-back + wait;
  append  — abo_append of the new point alone (its launches, its read-back + wait); trmv = the device time of its two mat-vecs;
  other   — the rest of the incremental call: handle creation / release around the append.
Then a k sweep places the crossover rule of abo_update (include/abo_hip.h): k sequential abo_append against one refit of N + k points,
at N = 1024 and 8192.  Writes update_latency.{json,txt} into --out (default profiles/).

    python tools/update_latency.py [--iters 50] [--warmup 5] [--sizes 1024,8192,16384] [--out DIR]
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


def model(n_max, incremental):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE, device=0, n_max=n_max,
                             incremental_update=incremental)


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.asarray(v)
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "n": int(v.size)}


def loop(N0, iters, warmup):
    total = warmup + iters
    X = synth.points(11, N0 + total + 1, D)
    y = synth.objective(X, 0.05)
    cap = N0 + total + 128
    plain = model(0, False)
    cur = abo.update(model(cap, True), X[:N0], y[:N0])
    rec = {k: [] for k in ("refit", "incremental", "match", "append", "trmv", "other")}
    paths = set()
    for it in range(total):
        n = N0 + it
        _, t_ref = ms(lambda: abo.update(plain, X[:n + 1], y[:n + 1]))
        same, t_match = ms(lambda: abo.update(cur, X[:n], y[:n]))
        assert same.update_path == "shared"
        del same
        a, t_app = ms(lambda: abo.append(cur, X[n], y[n]))
        trmv = a.timings()["append_trmv_ms"]
        del a                                     # its rows go back: the update below appends in place
        nxt, t_inc = ms(lambda: abo.update(cur, X[:n + 1], y[:n + 1]))
        paths.add(nxt.update_path)
        cur = nxt
        if it >= warmup:
            rec["refit"].append(t_ref); rec["incremental"].append(t_inc); rec["match"].append(t_match)
            rec["append"].append(t_app); rec["trmv"].append(trmv); rec["other"].append(t_inc - t_match - t_app)
    assert paths == {"appended"}, paths
    out = {k: stats(v) for k, v in rec.items()}
    out["speedup_median"] = out["refit"]["median"] / out["incremental"]["median"]
    out["match_bytes"] = 8.0 * N0 * (D + 1)
    out["trmv_bytes"] = 8.0 * N0 * N0
    return out


def sweep(N, ks, reps):
    X = synth.points(12, N + max(ks), D)
    y = synth.objective(X, 0.05)
    plain = model(0, False)
    base = abo.update(model(N + max(ks) + 128, False), X[:N], y[:N])
    rows = []
    for k in ks:
        ta, tr = [], []
        for r in range(reps + 1):
            def chain():
                m = base
                for j in range(k):
                    m = abo.append(m, X[N + j], y[N + j])
                return m
            m, t = ms(chain)
            del m
            _, t2 = ms(lambda: abo.update(plain, X[:N + k], y[:N + k]))
            if r:
                ta.append(t); tr.append(t2)
        rows.append({"k": k, "appends_ms": float(np.median(ta)), "refit_ms": float(np.median(tr)),
                     "ratio": float(np.median(ta) / np.median(tr))})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1024,8192,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory of the record")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = {"d": D, "kernel": "Matern52", "noise": NOISE, "device": torch.cuda.get_device_name(0), "loop": {}, "k_sweep": {}}
    lines = [f"update(model, xs, ys): refit vs incremental (abo_update), d = {D}, Matern-5/2, {a.iters} iterations after "
             f"{a.warmup} warm-up, alternated in one process; ms per call (median [p10, p90])"]
    for N0 in [int(s) for s in a.sizes.split(",")]:
        r = loop(N0, a.iters, a.warmup)
        res["loop"][str(N0)] = r
        f = lambda k: f"{r[k]['median']:.3f} [{r[k]['p10']:.3f}, {r[k]['p90']:.3f}]"
        lines.append(f"N0={N0:6d}  refit {f('refit')}  incremental {f('incremental')}  speed-up {r['speedup_median']:.1f}x")
        lines.append(f"          incremental = match {f('match')} + append {f('append')} (trmv device {f('trmv')}) "
                     f"+ other {f('other')}")
        print(lines[-2]); print(lines[-1]); sys.stdout.flush()
    ks = [1, 2, 4, 8, 16, 32, 64]
    lines.append("k sweep: k sequential bordered appends vs one refit of N + k points (ms, median of "
                 f"{a.reps}); ratio < 1: appending is cheaper")
    for N in (1024, 8192):
        rows = sweep(N, ks, a.reps)
        res["k_sweep"][str(N)] = rows
        for row in rows:
            lines.append(f"N={N:6d} k={row['k']:3d}  appends {row['appends_ms']:8.3f}  refit {row['refit_ms']:8.3f}  ratio {row['ratio']:.3f}")
            print(lines[-1]); sys.stdout.flush()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "update_latency.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(a.out, "update_latency.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
