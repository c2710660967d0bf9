"""Latency of the ARD hyper-parameter gradient (abo_nlml_grad_ard) beside the isotropic one and beside what a host without it pays.

An objective evaluation of the ARD search (hyperparams.nlml_and_grad_ard) is one refit on coordinates divided by ℓ_c + abo_nlml_grad_ard:
K⁻¹ = WᵀW on the fp64 MFMA GEMM as for abo_nlml_grad, then ONE sweep over K⁻¹ − ααᵀ that yields all d traces.  Without the call a host
takes central differences of the NLML in each log ℓ_c: 2d + 1 refits per evaluation (value + 2 per coordinate; the scale's partial is
analytic from the value's own factor).

    python tools/ard_latency.py [N ...]        (default 1024 4096 8192; d = 8, Matérn-5/2)
Prints per N, measured in the same run: the ARD sweep and the isotropic sweep (abo_timings.nlml_trace_ms, HIP events) and their ratio,
the K⁻¹ product both are preceded by, a whole objective evaluation both ways (host wall clock, refit + gradient), and 2d + 1 refits.
Medians of 7 after 3 warm-up rounds.  Writes the same text to profiles/ard_latency.txt.
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth

sizes = [int(a) for a in sys.argv[1:]] or [1024, 4096, 8192]
d, REPS, WARM = 8, 7, 3
ELLS = np.logspace(-0.3, 0.3, d)
L = abo._lib.lib()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def evaluation(ard, X, y):
    """one objective evaluation → (wall ms, timings)"""
    t0 = time.perf_counter()
    k = abo.with_lengthscale(abo.Matern52Kernel(), ELLS if ard else 1.0)
    m = abo.update(abo.HipStandardGP(k, 1e-3), X, y)
    v, s = C.c_double(), C.c_double()
    if ard:
        g = (C.c_double * d)()
        abo._lib.check(L.abo_nlml_grad_ard(m._require(), d, C.byref(v), g, C.byref(s), None))
    else:
        g = C.c_double()
        abo._lib.check(L.abo_nlml_grad(m._require(), C.byref(v), C.byref(g), C.byref(s)))
    return (time.perf_counter() - t0) * 1e3, m.timings()


def refits(n, X, y):
    """n refits with the NLML value read back after each: what central differences are made of"""
    t0 = time.perf_counter()
    for i in range(n):
        k = abo.with_lengthscale(abo.Matern52Kernel(), ELLS * (1.0 + 1e-5 * (i - n // 2)))
        abo.nlml_fitted(abo.update(abo.HipStandardGP(k, 1e-3), X, y))
    return (time.perf_counter() - t0) * 1e3


say(f"ARD gradient latency: d = {d}, Matern-5/2, medians of {REPS} (after {WARM} warm-up rounds); sweeps from HIP events, evaluations host wall clock")
say("     N | K^-1 GEMM ms | sweep ms: ARD  isotropic  ratio | evaluation ms (refit + gradient): ARD  isotropic | "
    f"{2 * d + 1} refits ms (central differences) | ARD evaluation / refits")
for N in sizes:
    X, y = synth.standardized_problem(N, d, 0.03)
    rec = {"ard": [], "iso": [], "fd": []}
    for r in range(WARM + REPS):
        a, i, f = evaluation(True, X, y), evaluation(False, X, y), refits(2 * d + 1, X, y)
        if r >= WARM:
            rec["ard"].append(a); rec["iso"].append(i); rec["fd"].append(f)
    med = lambda xs: float(np.median(xs))
    sw_a, sw_i = med([t["nlml_trace_ms"] for _, t in rec["ard"]]), med([t["nlml_trace_ms"] for _, t in rec["iso"]])
    kinv = med([t["nlml_kinv_ms"] for _, t in rec["ard"]])
    ev_a, ev_i, fd = med([w for w, _ in rec["ard"]]), med([w for w, _ in rec["iso"]]), med(rec["fd"])
    say(f"{N:6d} | {kinv:12.3f} | {sw_a:13.3f}  {sw_i:9.3f}  {sw_a / sw_i:5.2f} | {ev_a:37.3f}  {ev_i:9.3f} | {fd:38.3f} | {ev_a / fd:6.3f}")
    assert ev_a < fd, f"N = {N}: an ARD objective evaluation ({ev_a:.3f} ms) must cost less than the {2 * d + 1} refits beside it ({fd:.3f} ms)"
with open(os.path.join(ROOT, "profiles", "ard_latency.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
