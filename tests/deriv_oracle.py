"""NumPy restatement of the (f, ∇f) posterior of a VALUE-ONLY GP (abo_predict_deriv) — TEST INFRASTRUCTURE ONLY, the checker of
tests/test_deriv_cpu.py and tests/test_gpu_deriv.py.

Built from the project's oracles alone: the fit is `oracle.gp_oracle.fit`; the cross block is the value rows of
`oracle.grad_oracle.grad_kernel_matrix(family, ℓ, σ_f², X, Z)` (K[:N, :], columns by outputs over Z), the prior block of a query point is
`grad_kernel_matrix(…, Z[j:j+1], Z[j:j+1])`;  μ = mean_vec + K_xzᵀα,  Σ_j = K_zz − V_jᵀV_j + 1e-18·I with V = L⁻¹K_xz, and the score is
`grad_oracle.grad_norm_ucb`'s formula on the gradient block.  Results are point-major: mu (M, p), cov (M, p, p), p = d + 1.
ARD (one length scale per coordinate) goes through tests/ard_oracle.py's scaling — ℓ = 1 on x_c/ℓ_c — and the chain rule back to the
caller's coordinates is applied HERE, independently of the package: ∂/∂x_c = (1/ℓ_c)·∂/∂x′_c."""
import math

import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as O
from oracle import grad_oracle as G
from tests import ard_oracle as A


def score_of(mu, cov, beta):
    """grad_oracle.grad_norm_ucb's expression, point by point, on point-major means and blocks"""
    out = np.empty(mu.shape[0])
    for j in range(mu.shape[0]):
        g, S = mu[j, 1:], cov[j, 1:, 1:]
        out[j] = -(g @ g + np.trace(S)) + beta * math.sqrt(max(4 * g @ S @ g + 2 * np.sum(S * S), 1e-12))
    return out


def from_state(st: O.GPState, Z, beta: float = 0.0):
    """(mu (M, p), cov (M, p, p), score (M,), prior (p,)) of the value-only state `st` at the points Z"""
    Z = O._as_points(Z)
    M, d = Z.shape
    N, p = st.X.shape[0], d + 1
    Kxz = G.grad_kernel_matrix(st.family, st.ell, st.sigma_f2, st.X, Z)[:N, :]          # (N, p·M), column q·M + j
    mean_vec = np.concatenate([[st.mean_c], np.zeros(d)])
    mu = (np.repeat(mean_vec, M) + Kxz.T @ st.alpha).reshape(p, M).T
    V = sla.solve_triangular(st.L, Kxz, lower=True, check_finite=False)
    cov = np.empty((M, p, p))
    for j in range(M):
        Vj = V[:, j + M * np.arange(p)]
        Kzz = G.grad_kernel_matrix(st.family, st.ell, st.sigma_f2, Z[j:j + 1], Z[j:j + 1])
        cov[j] = Kzz - Vj.T @ Vj + O.FINITE_GP_JITTER * np.eye(p)
    return np.ascontiguousarray(mu), cov, score_of(mu, cov, beta), G.prior_var(st.family, st.ell, st.sigma_f2, d)


def posterior(family, ell, sigma_f2, noise_var, mean_c, X, y, Z, beta: float = 0.0):
    return from_state(O.fit(family, ell, sigma_f2, noise_var, mean_c, X, y), Z, beta)


def posterior_ard(family, ells, sigma_f2, noise_var, mean_c, X, y, Z, beta: float = 0.0):
    """the same for one length scale per coordinate, in the CALLER's coordinates"""
    ells = np.asarray(ells, dtype=np.float64)
    st = A.fit(family, ells, sigma_f2, noise_var, mean_c, X, y)
    mu, cov, _, prior = from_state(st, A.scaled(Z, ells), beta)
    dinv = np.concatenate([[1.0], 1.0 / ells])
    mu = mu * dinv
    cov = cov * np.outer(dinv, dinv)
    return mu, cov, score_of(mu, cov, beta), prior * dinv * dinv
