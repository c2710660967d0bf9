"""NumPy restatement of the ARD kernel (one length scale per coordinate) — TEST INFRASTRUCTURE ONLY, the checker of
tests/test_ard_cpu.py and tests/test_gpu_ard.py.

k(x,z) = σ_f²·κ(‖(x − z)./ℓ‖) is the isotropic kernel with ℓ = 1 on the coordinates x_c/ℓ_c (KernelFunctions builds it the same way:
kernel ∘ ARDTransform(1 ./ ℓ)), so value-side quantities are `oracle.gp_oracle` on scaled inputs.  The analytic gradient is computed
densely (N × N × d): ∂NLML/∂θ = ½ tr((K⁻¹ − ααᵀ) ∂K/∂θ) with ∂K_ij/∂log ℓ_c = σ_f²·q(d2_ij)·e_ijc², e = (x_i − x_j)./ℓ, d2 = Σ_c e_c²,
q(d2) = −κ'(r)/r in closed form (r = √d2); ∂K/∂log σ_f² = K − σ²I; ∂K/∂log σ² = σ²I."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O


def scaled(X, ells):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    return X / np.asarray(ells, dtype=np.float64)


def fit(family, ells, sigma_f2, noise_var, mean_c, X, y):
    """the oracle's state of the ARD model: `oracle.gp_oracle.fit` on scaled inputs with ℓ = 1"""
    return O.fit(family, 1.0, sigma_f2, noise_var, mean_c, scaled(X, ells), y)


def nlml(family, ells, sigma_f2, noise_var, mean_c, X, y) -> float:
    return O.nlml(fit(family, ells, sigma_f2, noise_var, mean_c, X, y))


def q_profile(family, d2):
    """(∂κ/∂log ℓ)/d2 on the squared scaled distance, finite at 0"""
    d2 = np.asarray(d2, dtype=np.float64)
    if family == O.SE:
        return np.exp(-0.5 * d2)
    r = np.sqrt(d2)
    if family == O.MATERN32:
        return 3.0 * np.exp(-math.sqrt(3.0) * r)
    if family == O.MATERN52:
        s5 = math.sqrt(5.0)
        return (5.0 / 3.0) * (1.0 + s5 * r) * np.exp(-s5 * r)
    if family == O.MATERN72:
        s7 = math.sqrt(7.0)
        return (7.0 / 5.0 + 7.0 * s7 / 5.0 * r + 49.0 / 15.0 * d2) * np.exp(-s7 * r)
    raise ValueError(f"unknown kernel family {family}")


def nlml_and_grad(family, ells, sigma_f2, noise_var, mean_c, X, y):
    """(nlml, ∂/∂log ℓ_c (d,), ∂/∂log σ_f², ∂/∂log σ²), dense"""
    st = fit(family, ells, sigma_f2, noise_var, mean_c, X, y)
    Xs = st.X
    N = Xs.shape[0]
    E2 = (Xs[:, None, :] - Xs[None, :, :]) ** 2                     # (N, N, d)
    d2 = E2.sum(-1)
    Kinv = sla.cho_solve((st.L, True), np.eye(N))
    M = Kinv - np.outer(st.alpha, st.alpha)
    W = M * (sigma_f2 * q_profile(family, d2))
    g_ell = 0.5 * np.einsum("ij,ijc->c", W, E2)
    K = sigma_f2 * O.kappa(family, d2)
    g_sf2 = 0.5 * float(np.sum(M * K))
    g_noise = 0.5 * noise_var * float(np.trace(M))
    return O.nlml(st), g_ell, g_sf2, g_noise


def central_differences(family, ells, sigma_f2, noise_var, mean_c, X, y, h=1e-5):
    """central differences of the oracle's NLML in each log ℓ_c, in log σ_f² and in log σ² (None when σ² = 0)"""
    ells = np.asarray(ells, dtype=np.float64)

    def f(le, ls, ln):
        return nlml(family, np.exp(le), math.exp(ls), (math.exp(ln) if noise_var > 0 else 0.0), mean_c, X, y)

    le, ls = np.log(ells), math.log(sigma_f2)
    ln = math.log(noise_var) if noise_var > 0 else 0.0
    g_ell = np.array([(f(le + h * e, ls, ln) - f(le - h * e, ls, ln)) / (2 * h) for e in np.eye(ells.shape[0])])
    g_sf2 = (f(le, ls + h, ln) - f(le, ls - h, ln)) / (2 * h)
    g_noise = (f(le, ls, ln + h) - f(le, ls, ln - h)) / (2 * h) if noise_var > 0 else None
    return g_ell, g_sf2, g_noise


def two_coordinate_problem(seed: int, N: int = 80, d: int = 4):
    """(X, y): N points in [0,1)^d and a standardised objective that depends on the first two coordinates only — the case of the ARD
    hyper-parameter search tests (the other coordinates are irrelevant: their length scales should end long)"""
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(5.0 * X[:, 0]) + np.cos(4.0 * X[:, 1]) * (1.0 + X[:, 0]) + 0.01 * rng.standard_normal(N)
    return X, (y - y.mean()) / y.std(ddof=1)


def stub_nlml_and_grad_ard(model, params, xs, ys):
    """`hyperparams.nlml_and_grad_ard` answered by this helper instead of the device (same signature and parameter order)"""
    p = np.asarray(params, dtype=np.float64)
    v, g_ell, g_sf2, _ = nlml_and_grad(model.kernel.family, np.exp(p[:-1]), math.exp(p[-1]), model.noise_var,
                                       float(getattr(model.mean, "c", 0.0)), xs, ys)
    return v, np.append(g_ell, g_sf2)


def stub_nlml_and_grad(model, params, xs, ys):
    """`hyperparams.nlml_and_grad` (isotropic) the same way: the sum of the per-coordinate partials at equal length scales"""
    X = np.asarray(xs, dtype=np.float64)
    d = 1 if X.ndim == 1 else X.shape[1]
    v, g = stub_nlml_and_grad_ard(model, [params[0]] * d + [params[1]], xs, ys)
    return v, np.array([g[:d].sum(), g[d]])
