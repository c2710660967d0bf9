"""Latency of the joint posterior covariance between point sets (abo_predict_cov) beside the only route without it.

Without the call a posterior covariance takes `get_factor`: read the N × N inverse factor L⁻¹ back to the host (N² doubles), generate
K_XZ there, V = L⁻¹K_XZ and cov = K_ab − V_aᵀV_b in NumPy.  abo_predict_cov keeps all of it on the device: K_ZX from the generator,
V = K_ZX·L⁻ᵀ and the signed product on the fp64 MFMA GEMM, Ma·Mb doubles read back.

    python tools/cov_latency.py [N ...]        (default 1024 4096 8192; d = 8, Matérn-5/2; Ma = Mb = 256 and 4096)
Prints per (N, M), all measured in the same run (host wall clock, medians; the device call 7 times after 3 warm-up rounds, the host
route 3 times after 1): the symmetric form cov(Z_a, Z_a) and the rectangular form cov(Z_a, Z_b) beside the host route for each, the
rate of the call's algorithmic flop, and the largest difference between the two routes.  Asserts only that the call is the faster of
the two.  Writes the same text to profiles/cov_latency.txt.
"""
import ctypes as C
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth

sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 8192]
d, REPS, WARM, HOST_REPS, HOST_WARM = 8, 7, 3, 3, 1
ELL, SF2, NOISE = 1.0, 1.0, 1e-3
L = abo._lib.lib()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def median_ms(f, reps, warm):
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        out = f()
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def matern52(A, B):
    """σ_f²·(1 + √5 r + 5 r²/3)·exp(−√5 r), r = ‖a − b‖/ℓ, differences formed directly"""
    d2 = np.zeros((A.shape[0], B.shape[0]))
    for c in range(A.shape[1]):
        e = A[:, c][:, None] / ELL - B[:, c][None, :] / ELL
        d2 += e * e
    r = np.sqrt(d2)
    return SF2 * (1.0 + math.sqrt(5.0) * r + 5.0 * d2 / 3.0) * np.exp(-math.sqrt(5.0) * r)


def host_route(m, X, za, zb):
    """what exists without the call: L⁻¹ read back (abo_get_factor), the rest in NumPy; zb None: the symmetric form"""
    N = X.shape[0]
    Li = np.empty((N, N))
    abo._lib.check(L.abo_get_factor(m._require(), None, None, Li.ctypes.data))
    Va = Li @ matern52(X, za)
    if zb is None:
        return matern52(za, za) - Va.T @ Va
    return matern52(za, zb) - Va.T @ (Li @ matern52(X, zb))


say(f"joint posterior covariance latency: d = {d}, Matern-5/2, host wall clock, medians (abo_predict_cov: {REPS} after {WARM} warm-up "
    f"rounds; host route: {HOST_REPS} after {HOST_WARM}), one run")
say("     N |    M | form        | abo_predict_cov ms  (TFLOP/s) | get_factor + NumPy ms | ratio | max |difference| / sigma_f2")
rng = np.random.default_rng(9)
for N in sizes:
    X, y = synth.standardized_problem(N, d, 0.03)
    m = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE), X, y)
    for M in (256, 4096):
        za, zb = rng.random((M, d)), rng.random((M, d))
        for form, b in (("symmetric", None), ("rectangular", zb)):
            t_dev, cov = median_ms(lambda: abo.posterior_cov(m, za, b), REPS, WARM)
            t_host, ref = median_ms(lambda: host_route(m, X, za, b), HOST_REPS, HOST_WARM)
            # algorithmic flop: the triangular V products (N²·M each) and the covariance product (2·M²·N, half of it in the symmetric form)
            flop = (1 if b is None else 2) * float(N) * N * M + (1.0 if b is None else 2.0) * float(M) * M * N
            diff = float(np.max(np.abs(cov - ref))) / SF2
            say(f"{N:6d} | {M:4d} | {form:11s} | {t_dev:19.3f}  ({flop / t_dev / 1e9:8.2f}) | {t_host:21.1f} | {t_dev / t_host:5.3f} | {diff:.2e}")
            assert t_dev < t_host, f"N = {N}, M = {M}, {form}: abo_predict_cov ({t_dev:.3f} ms) must beat the host route ({t_host:.1f} ms)"
with open(os.path.join(ROOT, "profiles", "cov_latency.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
