"""NumPy/SciPy checker of the knowledge gradient over a discrete decision set — TEST INFRASTRUCTURE ONLY (tests/test_kg_cpu.py,
tests/test_gpu_kg.py, tools/kg_latency.py), on top of `oracle.gp_oracle` and `tests.cov_oracle`.  Nothing here reads the code under test.

    KG = E[max_j (a_j + b_j·Z)] − max_j a_j,   Z ~ N(0, 1)

`kg_lines` is Frazier, Powell and Dayanik (2009), Algorithm 1: sort by (b, a) ascending, of equal slopes keep the largest intercept, one
stack scan for the upper envelope (line i enters with the breakpoint c = (a_top − a_i)/(b_i − b_top); while c ≤ the breakpoint under the
top, pop), then KG = Σ_t (b_{e_t} − b_{e_{t−1}})·h(−|c_t|) with h(z) = φ(z) + z·Φ(z) and Φ(z) = ½·erfc(−z/√2) at z ≤ 0 — every term ≥ 0.
`kg_quadrature` is an independent second evaluation: the trapezoid rule on E[max] itself.  `kg_model` is the KG of a GP from
cov_oracle / gp_oracle quantities (minimisation: a = −μ, b = cov/sqrt(v + σ_n²))."""
import math

import numpy as np
from scipy.special import erfc

from oracle import gp_oracle as O
from tests import cov_oracle as CO

VAR_FLOOR = 1e-12
INV_SQRT_2PI = 0.3989422804014327
TIE_ULPS = 4


def h(z):
    """φ(z) + z·Φ(z) at z ≤ 0; where Φ underflows to 0 the product is 0 (z = −Inf)"""
    z = float(z)
    Phi = 0.5 * float(erfc(-z * math.sqrt(0.5)))
    return INV_SQRT_2PI * math.exp(-0.5 * z * z) + (0.0 if Phi == 0.0 else z * Phi)


def _div(x, y):
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        return float(np.float64(x) / np.float64(y))


def envelope(a, b):
    """(a, b, c, tie) of the upper envelope of the lines a_j + b_j·z in order of slope: c[t] the breakpoint between lines t − 1 and t
    (c[0] = −Inf); tie: some pop decision compared two breakpoints within TIE_ULPS ulp of each other (the count is then not defined
    to rounding)"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    order = np.lexsort((a, b))                                   # by b, then a, ascending
    a, b = a[order], b[order]
    keep = np.append(b[1:] != b[:-1], True)                      # of equal slopes the last one: the largest intercept
    a, b = a[keep], b[keep]
    sa, sb, sc = [], [], []
    tie = False
    for ai, bi in zip(a, b):
        while True:
            if not sa:
                c = -math.inf
                break
            c = _div(sa[-1] - ai, bi - sb[-1])
            if len(sa) == 1:
                break
            if abs(c - sc[-1]) <= TIE_ULPS * np.spacing(max(abs(c), abs(sc[-1]))):
                tie = True
            if c <= sc[-1]:
                sa.pop(), sb.pop(), sc.pop()
            else:
                break
        sa.append(float(ai)), sb.append(float(bi)), sc.append(c)
    return np.array(sa), np.array(sb), np.array(sc), tie


def kg_lines(a, b, with_count=False):
    """KG of one row of lines; NaN (count 0) when any a or b is not finite"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(b))):
        return (math.nan, 0, False) if with_count else math.nan
    ea, eb, ec, tie = envelope(a, b)
    s = 0.0
    for t in range(1, len(ea)):
        s += (eb[t] - eb[t - 1]) * h(-abs(ec[t]))
    return (s, len(ea), tie) if with_count else s


def kg_rows(a, B, self_a=None, self_b=None):
    """(val [Ma], nenv [Ma], tie [Ma]) of the rows of B against the shared intercepts a; self_a / self_b: one more line per row"""
    B = np.asarray(B, dtype=np.float64)
    val, nenv, tie = np.empty(B.shape[0]), np.empty(B.shape[0], dtype=np.int64), np.zeros(B.shape[0], dtype=bool)
    for i in range(B.shape[0]):
        ai, bi = np.asarray(a, dtype=np.float64), B[i]
        if self_a is not None:
            ai, bi = np.append(ai, self_a[i]), np.append(bi, self_b[i])
        val[i], nenv[i], tie[i] = kg_lines(ai, bi, with_count=True)
    return val, nenv, tie


def kg_quadrature(a, b, n=400001, zmax=12.0):
    """E[max_j (a_j + b_j·Z)] − max_j a_j by the trapezoid rule on [−zmax, zmax] (the integrand is piecewise smooth with Gaussian tails:
    error ~ 1e-10·max|b| at this step, beyond 12 σ nothing is left in float64); the maximum is taken against the largest intercept
    first, so that the integrand is max_j(…) − a_max ≥ … evaluated without cancellation of a large common offset"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    z = np.linspace(-zmax, zmax, n)
    a0 = a.max()
    m = np.full(n, -np.inf)
    for aj, bj in zip(a - a0, b):
        np.maximum(m, aj + bj * z, out=m)
    w = INV_SQRT_2PI * np.exp(-0.5 * z * z)
    f = m * w
    dz = z[1] - z[0]
    return float(dz * (f.sum() - 0.5 * (f[0] + f[-1])))


def kg_from_posterior(mu_b, cov, v, noise, mu_a=None):
    """KG per candidate from the decision set's means, the Ma × Mb latent covariance, the candidates' latent variances and the noise;
    mu_a given: the candidate's own line (−mu_a[i], v_i/sqrt(v_i + noise)) joins row i.  v_i + noise ≤ 1e-12: 0.0."""
    cov = np.asarray(cov, dtype=np.float64)
    ma = cov.shape[0]
    val, nenv, tie = np.zeros(ma), np.ones(ma, dtype=np.int64), np.zeros(ma, dtype=bool)
    a = -np.asarray(mu_b, dtype=np.float64)
    for i in range(ma):
        x = v[i] + noise
        if x <= VAR_FLOOR:
            continue
        den = math.sqrt(x)
        ai, bi = a, cov[i] / den
        if mu_a is not None:
            ai, bi = np.append(a, -mu_a[i]), np.append(bi, v[i] / den)
        val[i], nenv[i], tie[i] = kg_lines(ai, bi, with_count=True)
    return val, nenv, tie


def kg_model(family, ell, sigma_f2, noise_var, mean_c, X, y, za, zb=None, noise=None, include_self=False):
    """KG of the candidates za over the decision set zb (None: za itself, the symmetric form) under the GP (family, ell, sigma_f2,
    noise_var, mean_c) conditioned on (X, y); noise None: noise_var.  → (val, nenv, tie)"""
    noise = noise_var if noise is None else noise
    if zb is None:
        mu, cov = CO.mean_and_cov(family, ell, sigma_f2, noise_var, mean_c, X, y, za)
        return kg_from_posterior(mu, cov, np.diag(cov), noise)
    mu_b, _ = CO.mean_and_cov(family, ell, sigma_f2, noise_var, mean_c, X, y, zb)
    mu_a, cov_aa = CO.mean_and_cov(family, ell, sigma_f2, noise_var, mean_c, X, y, za)
    cov = CO.posterior_cov(family, ell, sigma_f2, noise_var, X, za, zb)
    return kg_from_posterior(mu_b, cov, np.diag(cov_aa), noise, mu_a=mu_a if include_self else None)


def top_k(scores, k):
    """the library's order: descending, ties to the lowest index, NaN first (Julia's sortperm(scores; rev=true) prefix)"""
    return O.top_k(np.asarray(scores, dtype=np.float64), k)


# ---- the GP cases both test files use: (N, d, noise, ell); candidates Za (130) against the decision set Zb (257) in [−0.1, 1.1]^d, Zb's
# ---- first three points copied from Za
SF2, MEAN_C = 1.7, 0.3
MA, MB = 130, 257
# The objective is small against the model's noise — 0.03·sin(2πx) summed over the coordinates plus 0.03·N(0, 1) around the prior mean, under
# σ² = 1e-2 —, so that the posterior means of the decision set lie within a few slopes of each other and most rows have a real envelope:
# tests/test_kg_cpu.py asserts that condition.  With synth.objective at its full amplitude only the candidates next to the one minimum
# (and those outside the data) have KG above 1e-6·√σ_f²; the (128, 1) case then meets the condition at no length scale.  ℓ of that
# case is 0.1, not the 0.05 first proposed: at 0.05 the median envelope of the form without the own line holds 3 lines.
GP_CASES = [(130, 3, 1e-2, 0.3), (128, 1, 1e-2, 0.1), (40, 2, 1e-2, 0.25)]
OBJ_AMPLITUDE, OBJ_NOISE_STD = 0.03, 0.03


def gp_problem(N, d):
    from abstractbayesopt.jl_amd import synth
    X = synth.points(1, N, d)
    return X, OBJ_AMPLITUDE * synth.objective(X, 0.0) + OBJ_NOISE_STD * synth.normal(3, 0, N) + MEAN_C


def gp_queries(d):
    rng = np.random.default_rng(17)
    za, zb = rng.random((MA, d)) * 1.2 - 0.1, rng.random((MB, d)) * 1.2 - 0.1
    zb[:3] = za[:3]
    return za, zb
