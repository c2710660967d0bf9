"""Latency of the knowledge gradient over a discrete decision set (abo_acq_kg) beside abo_predict_cov alone and beside the host route.

    python tools/kg_latency.py [N ...]        (default 1024 8192; d = 8, Matérn-5/2; Ma = Mb = 1024, 4096 and 8192)
Per (N, M) and form (symmetric: the decision set is the candidates; rectangular: a second set of M points, own line added), all measured
in the same run, host wall clock around calls that end in a stream synchronisation, medians (7 after 3 warm-up rounds), inputs and
outputs in device memory so that no transfer is timed:
  * abo_acq_kg, and abo_predict_cov alone at the same shapes — the difference is the KG stage (variances, row kernel);
  * the host route: abo_predict_cov read back to the host (Ma·Mb doubles) plus the NumPy checker (tests/kg_oracle.py) on the rows.  The
    checker is a Python loop; beyond M = 1024 it runs on the first 64 rows only and its time is scaled by Ma/64 — the column says so;
  * the largest difference between the device's values and the checker's on the rows the checker ran, and the median number of lines
    on the upper envelope over those rows.
Nothing is asserted: the figures are the result.  Writes the same text to profiles/kg_latency.txt.
"""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from tests import kg_oracle as K

sizes = [int(a) for a in sys.argv[1:]] or [1024, 8192]
d, REPS, WARM = 8, 7, 3
ELL, SF2, NOISE = 0.5, 1.0, 1e-2
HOST_ROWS = 64
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def median_ms(f, reps, warm):
    ts = []
    for r in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def host_route(m, za, zb, rows):
    """the covariance block read back, then the checker on `rows` rows → (values, envelope sizes, seconds of the read-back, of the rows)"""
    t0 = time.perf_counter()
    if zb is None:
        mu, cov = abo.mean_and_cov(m, za)
        mu_a, mu_b, v = mu, mu, np.diag(cov)
    else:
        cov = abo.posterior_cov(m, za, zb)
        mu_a, v = abo.mean_and_var(m, za)
        mu_b = abo.posterior_mean(m, zb)
    t1 = time.perf_counter()
    val, nenv, _ = K.kg_from_posterior(mu_b, cov[:rows], v[:rows], NOISE, mu_a=None if zb is None else mu_a[:rows])
    return val, nenv, t1 - t0, time.perf_counter() - t1


say(f"knowledge gradient latency: d = {d}, Matern-5/2, ell = {ELL}, noise = {NOISE}; host wall clock around synchronised calls, medians "
    f"({REPS} after {WARM} warm-up rounds), device inputs and outputs, one run")
say("     N |    M | form        | abo_acq_kg ms | abo_predict_cov ms | KG stage ms | host route ms (read-back + checker)      | "
    "max |difference| | median envelope lines")
rng = np.random.default_rng(9)
for N in sizes:
    X, y = synth.standardized_problem(N, d, 0.03)
    m = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE), X, y)
    for M in (1024, 4096, 8192):
        za, zb = rng.random((M, d)), rng.random((M, d))
        zat, zbt = torch.from_numpy(za).cuda(), torch.from_numpy(zb).cuda()
        for form, b, bt in (("symmetric", None, None), ("rectangular", zb, zbt)):
            t_kg, sc = median_ms(lambda: abo.knowledge_gradient(m, zat, bt), REPS, WARM)
            t_cov, _ = median_ms(lambda: abo.posterior_cov(m, zat, bt), REPS, WARM)
            rows = M if M <= 1024 else HOST_ROWS
            val, nenv, t_back, t_rows = host_route(m, za, b, rows)
            t_host = (t_back + t_rows * (M / rows)) * 1e3
            how = "all rows" if rows == M else f"{rows} rows x {M // rows}"
            diff = float(np.max(np.abs(sc[:rows].cpu().numpy() - val)))
            say(f"{N:6d} | {M:4d} | {form:11s} | {t_kg:13.3f} | {t_cov:18.3f} | {t_kg - t_cov:11.3f} | {t_host:12.1f} ({t_back * 1e3:8.1f} + checker, "
                f"{how:13s}) | {diff:16.2e} | {float(np.median(nenv)):.1f}")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "kg_latency.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
