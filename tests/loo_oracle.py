"""NumPy checker of leave-one-out cross-validation — TEST INFRASTRUCTURE ONLY (tests/test_loo_cpu.py, tests/test_gpu_loo.py), on top of
`oracle.gp_oracle`'s kernel matrix.

`brute_force` is the definition: for each i, condition on the other N − 1 points and predict y_i with the noise included.  It is the
reference for the values; nothing here reads the code under test.  `closed_form` is Rasmussen & Williams §5.4.2 from a dense inverse,
and `nlpl_and_grad` their eq. 5.13 densely:
    ∂(−nlpl)/∂θ = Σ_i [α_i r_i − ½(1 + α_i²/B_ii) s_i]/B_ii,   B = K̃⁻¹,  r = B (∂K/∂θ) α,  s_i = [B (∂K/∂θ) B]_ii
with ∂K/∂log ℓ = σ_f²·q(d2)·d2 (q = tests.ard_oracle.q_profile), ∂K/∂log σ_f² = K̃ − σ²I, ∂K/∂log σ² = σ²I."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O
from tests import ard_oracle as A

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _lpd(y, mu, var):
    return -0.5 * np.log(var) - (y - mu) ** 2 / (2.0 * var) - HALF_LOG_2PI


def brute_force(family, ell, sigma_f2, noise_var, mean_c, X, y):
    """(mu, var, lpd, nlpl) by N refits on N − 1 points each; N = 1: the prior (mean_c, σ_f² + σ²)"""
    X = O._as_points(X)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    N = X.shape[0]
    mu, var = np.empty(N), np.empty(N)
    for i in range(N):
        keep = np.arange(N) != i
        if N == 1:
            mu[i], var[i] = mean_c, sigma_f2 + noise_var
            continue
        st = O.fit(family, ell, sigma_f2, noise_var, mean_c, X[keep], y[keep])
        k = O.kernel_matrix(family, ell, sigma_f2, st.X, X[i:i + 1])[:, 0]
        v = sla.solve_triangular(st.L, k, lower=True, check_finite=False)
        mu[i] = mean_c + float(k @ st.alpha)
        var[i] = sigma_f2 + noise_var - float(v @ v)
    lpd = _lpd(y, mu, var)
    return mu, var, lpd, -float(np.sum(lpd))


def _dense(family, ell, sigma_f2, noise_var, mean_c, X, y):
    X = O._as_points(X)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    K = O.kernel_matrix(family, ell, sigma_f2, X)
    Kt = K + noise_var * np.eye(X.shape[0])
    B = np.linalg.inv(Kt)
    B = 0.5 * (B + B.T)
    return X, y, K, B, B @ (y - mean_c)


def closed_form(family, ell, sigma_f2, noise_var, mean_c, X, y):
    """(mu, var, lpd, nlpl) from the diagonal of the dense inverse"""
    X, y, K, B, alpha = _dense(family, ell, sigma_f2, noise_var, mean_c, X, y)
    b = np.diag(B)
    mu, var = y - alpha / b, 1.0 / b
    lpd = _lpd(y, mu, var)
    return mu, var, lpd, -float(np.sum(lpd))


def nlpl(family, ell, sigma_f2, noise_var, mean_c, X, y) -> float:
    return closed_form(family, ell, sigma_f2, noise_var, mean_c, X, y)[3]


def nlpl_and_grad(family, ell, sigma_f2, noise_var, mean_c, X, y):
    """(nlpl, ∂/∂log ℓ, ∂/∂log σ_f², ∂/∂log σ²), dense"""
    X, y, K, B, alpha = _dense(family, ell, sigma_f2, noise_var, mean_c, X, y)
    b = np.diag(B)
    d2 = O.sqdist(X, X, ell)
    dKs = (sigma_f2 * A.q_profile(family, d2) * d2, K, noise_var * np.eye(X.shape[0]))
    out = []
    for dK in dKs:
        Z = B @ dK
        r, s = Z @ alpha, np.einsum("ij,ji->i", Z, B)
        out.append(-float(np.sum((alpha * r - 0.5 * (1.0 + alpha ** 2 / b) * s) / b)))
    return (closed_form(family, ell, sigma_f2, noise_var, mean_c, X, y)[3], *out)


def central_differences(family, ell, sigma_f2, noise_var, mean_c, X, y, h=1e-5):
    """central differences of `nlpl` in log ℓ, log σ_f² and log σ² (None when σ² = 0)"""
    def f(le, ls, ln):
        return nlpl(family, math.exp(le), math.exp(ls), (math.exp(ln) if noise_var > 0 else 0.0), mean_c, X, y)

    le, ls = math.log(ell), math.log(sigma_f2)
    ln = math.log(noise_var) if noise_var > 0 else 0.0
    g_ell = (f(le + h, ls, ln) - f(le - h, ls, ln)) / (2 * h)
    g_sf2 = (f(le, ls + h, ln) - f(le, ls - h, ln)) / (2 * h)
    g_noise = (f(le, ls, ln + h) - f(le, ls, ln - h)) / (2 * h) if noise_var > 0 else None
    return g_ell, g_sf2, g_noise
