"""NumPy/SciPy checker of the joint posterior covariance between point sets — TEST INFRASTRUCTURE ONLY (tests/test_cov_cpu.py,
tests/test_gpu_cov.py), on top of `oracle.gp_oracle`'s kernel matrix.  Nothing here reads the code under test.

    K = σ_f²κ(X, X) + σ²I,   cov(a, b) = K_ab − K_aX K⁻¹ K_Xb  through cho_factor / cho_solve,   mu = m + K_aX K⁻¹ (y − m)

the latent covariance (no observation noise), float64 throughout.  `posterior_cov(..., xb=None)` is the symmetric form: symmetrised
(the two solves differ in the last bit) and with AbstractGPs' FiniteGP jitter 1e-18 on its diagonal, as posterior_var carries it."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O


def _solve(family, ell, sigma_f2, noise_var, X):
    X = O._as_points(X)
    K = O.kernel_matrix(family, ell, sigma_f2, X) + noise_var * np.eye(X.shape[0])
    return X, sla.cho_factor(K, lower=True, check_finite=False)


def posterior_cov(family, ell, sigma_f2, noise_var, X, xa, xb=None):
    X, cf = _solve(family, ell, sigma_f2, noise_var, X)
    xa = O._as_points(xa)
    sym = xb is None
    xb = xa if sym else O._as_points(xb)
    Kxb = O.kernel_matrix(family, ell, sigma_f2, X, xb)
    Kax = O.kernel_matrix(family, ell, sigma_f2, xa, X)
    cov = O.kernel_matrix(family, ell, sigma_f2, xa, xb) - Kax @ sla.cho_solve(cf, Kxb, check_finite=False)
    if sym:
        cov = 0.5 * (cov + cov.T)
        cov[np.diag_indices_from(cov)] += O.FINITE_GP_JITTER
    return cov


def mean_and_cov(family, ell, sigma_f2, noise_var, mean_c, X, y, xa):
    X, cf = _solve(family, ell, sigma_f2, noise_var, X)
    alpha = sla.cho_solve(cf, np.asarray(y, dtype=np.float64).reshape(-1) - mean_c, check_finite=False)
    mu = mean_c + O.kernel_matrix(family, ell, sigma_f2, O._as_points(xa), X) @ alpha
    return mu, posterior_cov(family, ell, sigma_f2, noise_var, X, xa)
