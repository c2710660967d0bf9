"""CPU tests of the derivative posterior of a value-only model (abo_predict_deriv): the checker tests/deriv_oracle.py against finite
differences of INDEPENDENT oracles, the header / binding / shim entries of the new call, and its null-handle refusal without a device.

How the finite-difference bounds are derived (no tuning: everything below is computed from h, the kernel and the data).
A difference quotient is a linear functional of f, so its error against the derivative is one too: with δ the stencil
(δf = Σ_i w_i f(z + s_i·h·e_c)) and ∂ = ∂/∂z_c,
  * mean:        |δμ − ∂μ| = |⟨μ, (δ − ∂)k(·, z)⟩_H| ≤ ‖μ‖_H·sd_prior((δ − ∂)f),  ‖μ‖_H² = αᵀK_XX α  (reproducing property, Cauchy–Schwarz);
  * covariance:  the mixed second difference of the joint posterior covariance IS Cov_post(δ_c f, δ_c' f), so
                 |Cov_post(δ_c f, δ_c' f) − Cov_post(∂_c f, ∂_c' f)| ≤ sd(δ_c f − ∂_c f)·sd(δ_c' f) + sd(∂_c f)·sd(δ_c' f − ∂_c' f)
                 ≤ 2·sd_prior((δ − ∂)f)·sqrt(k″)   (conditioning only lowers a variance; Var δf ≤ k″ = Var ∂f: δ averages ∂ over a segment).
Var_prior((δ − ∂)f) = Σ_ij w_i w_j k((s_i − s_j)h) + 2Σ_i w_i k'(s_i h) + k″ is a closed form of the one-dimensional prior kernel
k(t) = σ_f²φ(t²/ℓ²) — O(h⁴) for the central first difference (the truncation O(h²) of the covariance check), O(h⁸) for the fourth-order
stencil (O(h³) / O(h⁵) in the variance for Matérn-5/2, whose |t|⁵ term it sees) — evaluated in long double; the terms are of size
k(0)·Σ|w_i w_j| and cancel, so 64 long-double round-offs of that size are added to it.
Rounding, O(ε/h) for the mean and O(ε/h²) for the covariance: every oracle value entering a stencil carries an absolute error of at most
η = 64·N·ε·cond·S — the first-order bound of a Cholesky solve, cond ≤ (N·σ_f² + σ²)/σ², S the size of the value (max|y − m| + |m| for a mean,
σ_f² for a covariance) — and the stencil multiplies it by Σ_i |w_i|."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from oracle import gp_oracle as O
from oracle import grad_oracle as G
from tests import cov_oracle as CO
from tests import deriv_oracle as D
from tests import kgen_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
EPS = 2.0 ** -53
SF2, NOISE, MEAN_C, ELL = 1.7, 1e-2, 0.3, 0.6
FAMILIES = (O.SE, O.MATERN52, O.MATERN72)


def k1d(family, t):
    """(k(t), k'(t)) of the prior along one coordinate, long double"""
    t = np.asarray(t, dtype=LD)
    p0, p1, _, _ = R.phis(family, t * t / LD(ELL) ** 2)
    return LD(SF2) * p0, LD(SF2) * p1 * 2 * t / LD(ELL) ** 2


def gap_sd(family, offsets, weights, h):
    """sd_prior(Σ_i w_i f(z + s_i h e_c) − ∂_c f(z)), with the long-double cancellation slack of the module text"""
    s, w = np.asarray(offsets, dtype=LD), np.asarray(weights, dtype=LD) / LD(h)
    kk = k1d(family, (s[:, None] - s[None, :]) * LD(h))[0]
    k2 = float(G.prior_var(family, ELL, SF2, 1)[1])
    var = (w[:, None] * w[None, :] * kk).sum() + 2 * (w * k1d(family, s * LD(h))[1]).sum() + LD(k2)
    slack = 64 * float(np.finfo(LD).eps) * SF2 * float(np.abs(w).sum()) ** 2
    return float(np.sqrt(max(float(var), 0.0) + slack)), k2


def problem(d, N=12):
    rng = np.random.default_rng(5 + d)
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(1)) + MEAN_C + 0.05 * rng.standard_normal(N)
    Z = rng.random((4, d)) * 1.2 - 0.1
    Z[0] = X[3]                                              # a query point equal to a training point
    return X, y, Z


def eta(N, size):
    return 64 * N * EPS * (N * SF2 + NOISE) / NOISE * size


@pytest.mark.parametrize("d", (1, 3))
@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_gradient_mean_against_fourth_order_differences(family, d):
    X, y, Z = problem(d)
    st = O.fit(family, ELL, SF2, NOISE, MEAN_C, X, y)
    mu = D.from_state(st, Z)[0]
    h, offs, wts = 1e-2, (-2.0, -1.0, 1.0, 2.0), (1.0 / 12, -8.0 / 12, 8.0 / 12, -1.0 / 12)
    sd, _ = gap_sd(family, offs, wts, h)
    K = O.kernel_matrix(family, ELL, SF2, X)
    trunc = float(np.sqrt(st.alpha @ K @ st.alpha)) * sd
    rnd = (18.0 / 12) / h * eta(X.shape[0], float(np.max(np.abs(st.delta))) + abs(MEAN_C))
    np.testing.assert_allclose(mu[:, 0], O.predict(st, Z)[0], rtol=0, atol=eta(X.shape[0], np.max(np.abs(st.delta)) + abs(MEAN_C)))
    for c in range(d):
        fd = sum(w * O.predict(st, Z + s * h * np.eye(d)[c])[0] for s, w in zip(offs, wts)) / h
        err = float(np.max(np.abs(fd - mu[:, c + 1])))
        print(f"family={family} d={d} c={c}: |fd - grad mu| = {err:.3e}, bound = {trunc:.3e} (truncation) + {rnd:.3e} (rounding)")
        assert err <= trunc + rnd


@pytest.mark.parametrize("d", (1, 3))
@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_gradient_covariance_against_second_differences(family, d):
    X, y, Z = problem(d)
    st = O.fit(family, ELL, SF2, NOISE, MEAN_C, X, y)
    _, cov, _, prior = D.from_state(st, Z)
    h = 2e-3
    sd, k2 = gap_sd(family, (-1.0, 1.0), (-0.5, 0.5), h)
    assert prior[0] == SF2 and np.allclose(prior[1:], k2, rtol=1e-15, atol=0)
    trunc = 2.0 * sd * np.sqrt(k2)                           # O(h²)
    rnd = eta(X.shape[0], SF2) / (h * h)                     # O(ε/h²): four values, weights 1/(4h²)
    E = np.eye(d)
    var = O.predict(st, Z)[1]
    np.testing.assert_allclose(cov[:, 0, 0], var, rtol=0, atol=eta(X.shape[0], SF2))
    for j in range(Z.shape[0]):
        for c in range(d):
            for c2 in range(d):
                a = np.stack([Z[j] + h * E[c], Z[j] - h * E[c]])
                b = np.stack([Z[j] + h * E[c2], Z[j] - h * E[c2]])
                g = CO.posterior_cov(family, ELL, SF2, NOISE, X, a, b)
                fd = (g[0, 0] - g[0, 1] - g[1, 0] + g[1, 1]) / (4 * h * h)
                err = abs(fd - cov[j, c + 1, c2 + 1])
                assert err <= trunc + rnd, (family, d, j, c, c2, err, trunc, rnd)
            # the mixed f/∇f entry: the first difference of the joint covariance in its second argument (the same two bounds, one stencil)
            b = np.stack([Z[j] + h * E[c], Z[j] - h * E[c]])
            g = CO.posterior_cov(family, ELL, SF2, NOISE, X, Z[j:j + 1], b)
            err = abs((g[0, 0] - g[0, 1]) / (2 * h) - cov[j, 0, c + 1])
            assert err <= sd * np.sqrt(SF2) + eta(X.shape[0], SF2) / h, (family, d, j, c, err)
    print(f"family={family} d={d}: bound = {trunc:.3e} (truncation) + {rnd:.3e} (rounding), k'' = {k2:.3f}")
    # symmetric blocks, the jitter on the diagonal, the score from the same block
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    mu = D.from_state(st, Z)[0]
    np.testing.assert_array_equal(D.from_state(st, Z, 2.0)[2], D.score_of(mu, cov, 2.0))


def test_ard_oracle_applies_the_chain_rule():
    """equal length scales: the ARD form equals the isotropic one; unequal: the gradient mean is the fourth-order difference quotient of
    the ARD oracle's mean in the CALLER's coordinates (bound as above, in the scaled coordinate: h/ℓ_c there, a factor 1/ℓ_c back)"""
    family, d = O.MATERN52, 3
    X, y, Z = problem(d)
    mu_i, cov_i, sc_i, _ = D.posterior(family, ELL, SF2, NOISE, MEAN_C, X, y, Z, 2.0)
    mu_a, cov_a, sc_a, _ = D.posterior_ard(family, [ELL] * d, SF2, NOISE, MEAN_C, X, y, Z, 2.0)
    np.testing.assert_allclose(mu_a, mu_i, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(cov_a, cov_i, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(sc_a, sc_i, rtol=1e-8, atol=1e-8)
    from tests import ard_oracle as A
    ells = np.array([0.3, 0.6, 1.2])
    mu = D.posterior_ard(family, ells, SF2, NOISE, MEAN_C, X, y, Z)[0]
    st = A.fit(family, ells, SF2, NOISE, MEAN_C, X, y)
    h, offs, wts = 1e-2, (-2.0, -1.0, 1.0, 2.0), (1.0 / 12, -8.0 / 12, 8.0 / 12, -1.0 / 12)
    K = O.kernel_matrix(family, 1.0, SF2, st.X)
    for c in range(d):
        fd = sum(w * O.predict(st, A.scaled(Z + s * h * np.eye(d)[c], ells))[0] for s, w in zip(offs, wts)) / h
        # in the scaled coordinate the step is h/ℓ_c and the unit length scale plays ELL's part: the bound of gap_sd at (h/ℓ_c)·ELL
        sd, _ = gap_sd(family, offs, wts, h / ells[c] * ELL)
        trunc = float(np.sqrt(st.alpha @ K @ st.alpha)) * sd * ELL / ells[c]
        rnd = (18.0 / 12) / h * eta(X.shape[0], float(np.max(np.abs(st.delta))) + abs(MEAN_C))
        assert float(np.max(np.abs(fd - mu[:, c + 1]))) <= trunc + rnd, (c, trunc, rnd)


# ---- header, binding, shim --------------------------------------------------------------------------------------------------------------
def test_header_binding_and_shim_carry_the_call():
    hdr = open(os.path.join(ROOT, "include", "abo_hip.h")).read()
    assert int(re.search(r"#define ABO_ABI_VERSION (\d+)", hdr).group(1)) == 7 == abo._lib.ABI_VERSION
    added = hdr[hdr.index("added within ABI 7 (backwards-compatible"):hdr.index("/* status codes */")]
    assert "abo_predict_deriv" in added
    i0, i1 = hdr.index("#ifdef ABO_TEST_HOOKS"), hdr.index("#endif /* ABO_TEST_HOOKS */")
    text = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    proto = re.search(r"\bint32_t\s+abo_predict_deriv\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
    assert proto and hdr.index("int32_t abo_predict_deriv(") < i0
    hook = re.search(r"\bint32_t\s+abo_test_kgen_deriv\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)
    assert hook and i0 < hdr.index("int32_t abo_test_kgen_deriv(") < i1
    assert "abo_predict_deriv" in abo._lib.EXPORTS and "abo_test_kgen_deriv" in abo._lib.TEST_EXPORTS
    lib = abo._lib.lib()
    assert len(lib.abo_predict_deriv.argtypes) == len(proto.group(1).split(",")) == 10
    assert len(lib.abo_test_kgen_deriv.argtypes) == len(hook.group(1).split(",")) == 19
    # the same argument types as the gradient-enhanced twin
    assert list(lib.abo_predict_deriv.argtypes) == list(lib.abo_predict_grad_cov.argtypes)
    jl = open(os.path.join(ROOT, "integration", "julia", "HipStandardGP.jl")).read()
    call = re.search(r"LIBABO\.abo_predict_deriv\((.*?)\)::Int32", jl, flags=re.S)
    assert call and call.group(1).count("::") == 10
    # the three limits of the call are said where a user reads them
    doc = hdr[hdr.rindex("/*", 0, hdr.index("int32_t abo_predict_deriv(")):hdr.index("int32_t abo_predict_deriv(")]
    for word in ("abo_mgpu", "abo_acq_terms", "abo_optimize_acquisition", "fp64"):
        assert word in doc, word


def test_null_handle_is_refused_without_a_device():
    lib = abo._lib.lib()
    out = np.full(4, np.nan)
    z = np.zeros(1)
    assert lib.abo_predict_deriv(None, z.ctypes.data, 1, 1, 0, 0.0, out.ctypes.data, None, None, 0) == abo._lib.ABO_EINVAL
    msg = abo._lib.last_error()
    assert "abo_predict_deriv" in msg and "null" in msg
    assert np.all(np.isnan(out))


def test_host_routes_value_only_models_and_refuses_sharded_ones():
    """no device: an unfitted model fails in _require, a sharded one with the TypeError of the other single-device surfaces; an ARD
    model is not refused (the chain rule is applied on the way out)"""
    m = abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE)
    for f in (abo.posterior_grad_mean, abo.posterior_grad_var, abo.posterior_grad_cov, lambda mm, x: abo.GradientNormUCB(2.0)(mm, x)):
        with pytest.raises(ValueError):
            f(m, np.zeros((2, 3)))

    class Sharded(abo.HipStandardGP):
        devices = (0, 1)

    s = object.__new__(Sharded)
    s.__dict__.update(m.__dict__)
    with pytest.raises(TypeError, match="sharded"):
        abo.posterior_grad_cov(s, np.zeros((2, 3)))
    with pytest.raises(TypeError):
        abo.evaluate(abo.GradientNormUCB(2.0), s, np.zeros((2, 3)))
    mu = np.array([[0.5, 1.0, -2.0]])
    cov = np.array([[[9.0, 0.0, 0.0], [0.0, 2.0, 0.5], [0.0, 0.5, 1.0]]])
    np.testing.assert_allclose(abo.gradnorm_ucb_host(mu, cov, 2.0), D.score_of(mu, cov, 2.0), rtol=1e-15)
