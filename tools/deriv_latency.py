"""Latency of the derivative posterior of a value-only model (abo_predict_deriv) beside what exists without it.

    python tools/deriv_latency.py [N ...]        (default 1024 8192; d = 8, Matérn-5/2, M = 10 000 query points)
Per N, all in the same run, points and outputs in device memory (host wall clock around calls that end in a stream wait; medians of 7
after 3 warm-up rounds):
  * abo_predict_deriv: mean, p × p covariance block and GradientNormUCB score of every point (p = d + 1 = 9), with the phase split of
    abo_get_timings (generator / fp64 GEMM / per-point epilogue, device events) of the last round;
  * abo_predict, mean + variance, on the same handle (contraction="fp64") at the same M: one row of V per point where the call above
    contracts p — the ratio printed is expected near p, and is reported, not asserted;
  * the 2d abo_predict mean-only calls a central difference of the mean needs (which gives ∇μ alone: no covariance).
Writes the same text to profiles/deriv_latency.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from abstractbayesopt.jl_amd._lib import DEVICE

sizes = [int(a) for a in sys.argv[1:]] or [1024, 8192]
d, M, REPS, WARM = 8, 10000, 7, 3
ELL, SF2, NOISE, H = 1.0, 1.0, 1e-3, 1e-4
L = abo._lib.lib()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def median_ms(f):
    ts = []
    for r in range(WARM + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        if r >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


p = d + 1
say(f"derivative posterior latency: d = {d} (p = {p}), Matern-5/2, M = {M}, fp64 contraction, device buffers; host wall clock, median "
    f"[min, max] of {REPS} after {WARM} warm-up rounds, one run")
for N in sizes:
    X, y = synth.standardized_problem(N, d, 0.03)
    m = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE, contraction="fp64"), X, y)
    h = m._require()
    z = torch.from_numpy(np.random.default_rng(9).random((M, d))).cuda()
    mu = torch.empty((M, p), dtype=torch.float64, device="cuda")
    cov = torch.empty((M, p, p), dtype=torch.float64, device="cuda")
    sc = torch.empty(M, dtype=torch.float64, device="cuda")
    mu1, var1 = torch.empty(M, dtype=torch.float64, device="cuda"), torch.empty(M, dtype=torch.float64, device="cuda")
    stencil = [z + s * H * torch.eye(d, dtype=torch.float64, device="cuda")[c] for c in range(d) for s in (1.0, -1.0)]
    stencil = [t.contiguous() for t in stencil]

    def deriv():
        abo._lib.check(L.abo_predict_deriv(h, z.data_ptr(), M, d, DEVICE, 2.0, mu.data_ptr(), cov.data_ptr(), sc.data_ptr(), DEVICE))

    def predict():
        abo._lib.check(L.abo_predict(h, z.data_ptr(), M, d, DEVICE, mu1.data_ptr(), var1.data_ptr(), DEVICE))

    def central():
        for t in stencil:
            abo._lib.check(L.abo_predict(h, t.data_ptr(), M, d, DEVICE, mu1.data_ptr(), None, DEVICE))

    t_d = median_ms(deriv)
    tm = m.timings()
    t_p = median_ms(predict)
    t_c = median_ms(central)
    flop = float(p) * M * float(N) * N                                  # the triangular product V = K·L⁻ᵀ, algorithmic
    say(f"N = {N}")
    say(f"  abo_predict_deriv                {t_d[0]:9.3f} ms [{t_d[1]:.3f}, {t_d[2]:.3f}]   ({flop / t_d[0] / 1e9:.2f} TFLOP/s of p·M·N²)")
    say(f"    phases of the last round (device events): generator {tm['acq_kxz_ms']:.3f} ms, GEMM {tm['acq_var_gemm_ms']:.3f} ms, "
        f"epilogue {tm['acq_finalize_ms']:.3f} ms, call {tm['acq_total_ms']:.3f} ms; {tm['var_gemm_launches']} chunks")
    say(f"  abo_predict (mean + variance)    {t_p[0]:9.3f} ms [{t_p[1]:.3f}, {t_p[2]:.3f}]   ratio deriv / predict = {t_d[0] / t_p[0]:.2f} (p = {p})")
    say(f"  {2 * d} abo_predict mean-only calls    {t_c[0]:9.3f} ms [{t_c[1]:.3f}, {t_c[2]:.3f}]   ratio deriv / central difference = {t_d[0] / t_c[0]:.2f}")
with open(os.path.join(ROOT, "profiles", "deriv_latency.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
