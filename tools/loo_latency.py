"""Latency of leave-one-out cross-validation (abo_loo, abo_loo_grad) beside what it replaces.

abo_loo reads the triangle of the resident L⁻ᵀ once (N²·4 bytes); without it the leave-one-out distribution of a fitted model takes N
refits, or one refit per perturbed parameter set when only the objective is wanted.  abo_loo_grad is abo_nlml_grad's K⁻¹ = WᵀW product
plus ∂K/∂log ℓ as a matrix and one full N³ product against it.  An evaluation of the LOO hyper-parameter objective is one refit +
abo_loo_grad; central differences in (log ℓ, log σ_f², log σ²) would take 7 evaluations of refit + abo_loo.

    python tools/loo_latency.py [N ...]        (default 1024 4096 8192; d = 8, Matérn-5/2)
Prints per N, all measured in the same run (host wall clock, medians of 7 after 3 warm-up rounds): abo_loo beside a refit (and the
rate of its one read), abo_loo_grad beside abo_nlml_grad, and a whole analytic evaluation beside the 7 it replaces.  Asserts only that
the analytic evaluation is the cheaper of the two.  Writes the same text to profiles/loo_latency.txt.
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
d, REPS, WARM, NFD = 8, 7, 3, 7
L = abo._lib.lib()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def ms(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def refit(X, y, ell=1.0, sf2=1.0, noise=1e-3):
    return abo.update(abo.HipStandardGP(sf2 * abo.with_lengthscale(abo.Matern52Kernel(), ell), noise), X, y)


def loo_value(m):
    v = C.c_double()
    abo._lib.check(L.abo_loo(m._require(), None, None, None, C.byref(v), abo._lib.HOST))
    return v.value


def loo_grad(m):
    o = [C.c_double() for _ in range(4)]
    abo._lib.check(L.abo_loo_grad(m._require(), *(C.byref(x) for x in o)))


def nlml_grad(m):
    o = [C.c_double() for _ in range(3)]
    abo._lib.check(L.abo_nlml_grad(m._require(), *(C.byref(x) for x in o)))


def central_differences(X, y):
    """the 7 evaluations (refit + abo_loo) of central differences in three parameters: the point itself and ± h in each"""
    h = 1e-5
    for e, s, n in [(0, 0, 0), (h, 0, 0), (-h, 0, 0), (0, h, 0), (0, -h, 0), (0, 0, h), (0, 0, -h)]:
        loo_value(refit(X, y, np.exp(e), np.exp(s), 1e-3 * np.exp(n)))


say(f"leave-one-out latency: d = {d}, Matern-5/2, host wall clock, medians of {REPS} (after {WARM} warm-up rounds), one run")
say("     N | refit ms | abo_loo ms  (GB/s of N^2*4 bytes) | abo_nlml_grad ms | abo_loo_grad ms | analytic evaluation ms (refit + abo_loo_grad) | "
    f"{NFD} x (refit + abo_loo) ms | ratio")
for N in sizes:
    X, y = synth.standardized_problem(N, d, 0.03)
    rec = {k: [] for k in ("refit", "loo", "nlml_grad", "loo_grad", "eval", "fd")}
    for r in range(WARM + REPS):
        t_fit, m = ms(lambda: refit(X, y))
        t_loo, _ = ms(lambda: loo_value(m))
        t_ng, _ = ms(lambda: nlml_grad(m))
        t_lg, _ = ms(lambda: loo_grad(m))
        t_ev, _ = ms(lambda: loo_grad(refit(X, y)))
        t_fd, _ = ms(lambda: central_differences(X, y))
        if r >= WARM:
            for k, t in zip(rec, (t_fit, t_loo, t_ng, t_lg, t_ev, t_fd)):
                rec[k].append(t)
    q = {k: float(np.median(v)) for k, v in rec.items()}
    say(f"{N:6d} | {q['refit']:8.3f} | {q['loo']:10.3f}  ({N * N * 4 / q['loo'] / 1e6:8.1f}) | {q['nlml_grad']:16.3f} | {q['loo_grad']:15.3f} | "
        f"{q['eval']:45.3f} | {q['fd']:24.3f} | {q['eval'] / q['fd']:5.3f}")
    assert q["eval"] < q["fd"], (f"N = {N}: an analytic LOO evaluation ({q['eval']:.3f} ms) must cost less than the {NFD} evaluations of central "
                                 f"differences beside it ({q['fd']:.3f} ms)")
with open(os.path.join(ROOT, "profiles", "loo_latency.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
