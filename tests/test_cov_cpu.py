"""Joint posterior covariance between point sets, host side — no device work.

The checker is tests/cov_oracle.py.  Here: the checker against closed forms (one training point; three points in d = 1 against an
explicit 3 × 3 inverse), the places that name the new entry point (header, ctypes binding, Julia shim), the host's argument checks
with the library made unreachable, and sample_joint with the device call answered by the checker."""
import math
import os
import re

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import surrogate as S
from oracle import gp_oracle as O
from tests import cov_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "integration", "julia", "PosteriorCov.jl")
HEADER = os.path.join(ROOT, "include", "abo_hip.h")
FAMILIES = [O.SE, O.MATERN52, O.MATERN72, O.MATERN32]
SF2, NOISE, MEAN_C, ELL = 1.7, 1e-2, 0.3, 0.6


def test_header_binding_and_shim_name_the_same_function():
    """The issue's prose counts 10 arguments; the prototype it gives — and the header — has 11 (gp, Za, Ma, Zb, Mb, d, z_space, mu_a,
    mu_b, cov, out_space).  The binding is held to the header."""
    from tests import test_julia_shim_cpu as J
    protos = J.c_prototypes()
    name = "abo_predict_cov"
    assert name in protos and name in abo._lib.EXPORTS
    assert protos[name] == [("abo_gp", 1), ("double", 1), ("int64_t", 0), ("double", 1), ("int64_t", 0), ("int32_t", 0), ("int32_t", 0),
                            ("double", 1), ("double", 1), ("double", 1), ("int32_t", 0)]
    import ctypes as C
    want = {("abo_gp", 1): C.c_void_p, ("double", 1): C.c_void_p, ("int64_t", 0): C.c_int64, ("int32_t", 0): C.c_int32}
    assert list(abo._lib.lib().abo_predict_cov.argtypes) == [want[p] for p in protos[name]]
    assert abo._lib.lib().abo_predict_cov.restype is C.c_int32
    calls = J.julia_calls(JL)
    assert len(calls) == 3 and {c[0] for c in calls} == {name}            # posterior_cov (two methods) and mean_and_cov: one call each
    code = J._strip_jl_comments(open(JL).read())
    assert len(re.findall(r"LIBABO\.\w+\(", code)) == len(calls)
    for _, types, ret, line in calls:
        assert ret == "Int32" and len(types) == len(protos[name]), line
        assert all(J.jl_matches_c(t, c) for t, c in zip(types, protos[name])), line
    assert 'include("PosteriorCov.jl")' in open(J.SHIMS[0]).read()
    jl = open(JL).read()
    for sig in (r"^function posterior_cov\(m::HipStandardGP, xa::AbstractVector\)", r"^function mean_and_cov\(m::HipStandardGP, xa::AbstractVector\)",
                r"^function posterior_cov\(m::HipStandardGP, xa::AbstractVector, xb::AbstractVector\)"):
        assert re.search(sig, jl, flags=re.M), sig
    for f in ("posterior_cov", "mean_and_cov", "sample_joint"):
        assert callable(getattr(abo, f))


def test_abi_version_stays_7_and_lists_the_call():
    hdr = open(HEADER).read()
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr) and abo._lib.ABI_VERSION == 7
    block = hdr[hdr.index("#define ABO_ABI_VERSION"):]
    block = block[:block.index("*/")]
    assert "abo_predict_cov" in block[block.index("added within ABI 7"):]


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_with_one_training_point(family):
    """N = 1: cov(a, b) = k(a, b) − k(a, x) k(x, b)/(k(x, x) + σ²)"""
    rng = np.random.default_rng(3)
    x, a, b = rng.random((1, 2)), rng.random((5, 2)), rng.random((4, 2))
    k = lambda u, v: O.kernel_matrix(family, ELL, SF2, u, v)
    want = k(a, b) - k(a, x) @ k(x, b) / (SF2 + NOISE)
    np.testing.assert_allclose(CO.posterior_cov(family, ELL, SF2, NOISE, x, a, b), want, rtol=0, atol=4e-16 * SF2)
    sym = CO.posterior_cov(family, ELL, SF2, NOISE, x, a)
    want_s = k(a, a) - k(a, x) @ k(x, a) / (SF2 + NOISE)
    np.testing.assert_allclose(sym, want_s + 1e-18 * np.eye(5), rtol=0, atol=4e-16 * SF2)
    assert np.array_equal(sym, sym.T)
    mu, cov = CO.mean_and_cov(family, ELL, SF2, NOISE, MEAN_C, x, [1.1], a)
    np.testing.assert_allclose(mu, MEAN_C + k(a, x)[:, 0] * (1.1 - MEAN_C) / (SF2 + NOISE), rtol=0, atol=1e-15)
    assert np.array_equal(cov, sym)


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_with_three_training_points_against_an_explicit_inverse(family):
    """N = 3, d = 1: K⁻¹ written out as adj(K)/det(K); the condition number of K is below 1e3 here, so 1e-13·σ_f² leaves two digits"""
    X = np.array([0.1, 0.55, 0.9])
    a, b = np.array([0.0, 0.3, 0.7, 1.2]), np.array([0.2, 0.55])
    K = O.kernel_matrix(family, ELL, SF2, X) + NOISE * np.eye(3)
    (p, q, r), (_, s, t), (_, _, u) = K
    det = p * (s * u - t * t) - q * (q * u - t * r) + r * (q * t - s * r)
    adj = np.array([[s * u - t * t, r * t - q * u, q * t - r * s],
                    [r * t - q * u, p * u - r * r, q * r - p * t],
                    [q * t - r * s, q * r - p * t, p * s - q * q]])
    k = lambda v, w: O.kernel_matrix(family, ELL, SF2, v, w)
    want = k(a, b) - k(a, X) @ (adj / det) @ k(X, b)
    np.testing.assert_allclose(CO.posterior_cov(family, ELL, SF2, NOISE, X, a, b), want, rtol=0, atol=1e-13 * SF2)


class _Unreachable:
    def __call__(self):
        raise AssertionError("the library was touched")


def _fitted_stub(model, d):
    """a model that looks conditioned on d-dimensional data without a device: what `update` leaves behind"""
    model._h = S._Handle(None)
    model._d = d
    return model


def test_host_checks_raise_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(abo._lib, "lib", _Unreachable())
    m = _fitted_stub(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ELL), NOISE), 3)
    x3, x2 = np.zeros((4, 3)), np.zeros((4, 2))
    for call in (lambda: abo.posterior_cov(m, x2), lambda: abo.posterior_cov(m, x3, x2), lambda: abo.posterior_cov(m, x2, x2),
                 lambda: abo.mean_and_cov(m, x2), lambda: abo.sample_joint(m, x2, 3)):
        with pytest.raises(abo.DimensionMismatch):
            call()
    ard = _fitted_stub(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), [0.5, 0.7, 0.9]), NOISE), 3)
    with pytest.raises(abo.DimensionMismatch):
        abo.posterior_cov(ard, x2)
    g = _fitted_stub(abo.HipGradientGP(abo.Matern52Kernel(), 4, 0.1), 3)
    sh = abo.HipShardedGP(abo.Matern52Kernel(), 0.1, devices=(0, 0))
    for bad, word in ((g, "gradient"), (sh, "sharded")):
        for call in (lambda: abo.posterior_cov(bad, x3), lambda: abo.mean_and_cov(bad, x3), lambda: abo.sample_joint(bad, x3, 2)):
            with pytest.raises(TypeError, match=word):
                call()
    with pytest.raises(ValueError, match="8192"):
        abo.posterior_cov(m, np.zeros((8193, 3)))
    with pytest.raises(ValueError, match="1 to 8192"):
        abo.posterior_cov(m, np.zeros((0, 3)))
    # and with everything in order the call does go to the library
    with pytest.raises(AssertionError, match="touched"):
        abo.posterior_cov(m, x3)


PROBLEM = dict(family=O.MATERN52, ell=0.4, noise=1e-2)


def _problem():
    rng = np.random.default_rng(11)
    X = rng.random((12, 2))
    return X, np.sin(3.0 * X[:, 0]) + X[:, 1]


def _stub_mean_and_cov(noise):
    X, y = _problem()

    def f(model, x):
        return CO.mean_and_cov(PROBLEM["family"], PROBLEM["ell"], SF2, noise, MEAN_C, X, y, x)
    return f


def _model(noise):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), PROBLEM["ell"]), noise, mean=abo.ConstMean(MEAN_C))


def test_sample_joint_shape_determinism_and_moments(monkeypatch):
    monkeypatch.setattr(S, "mean_and_cov", _stub_mean_and_cov(PROBLEM["noise"]))
    m = _model(PROBLEM["noise"])
    x = np.array([[0.2, 0.3], [0.25, 0.35], [0.8, 0.1], [1.3, 1.2]])          # two close points, one apart, one outside the data
    n = 20000
    s = abo.sample_joint(m, x, n, rng=np.random.default_rng(5))
    assert s.shape == (n, 4) and s.dtype == np.float64
    assert np.array_equal(s, abo.sample_joint(m, x, n, rng=np.random.default_rng(5)))
    assert np.array_equal(s, abo.sample_joint(m, x, n, rng=5))
    assert not np.array_equal(s, abo.sample_joint(m, x, n, rng=6))
    assert abo.sample_joint(m, x, 0).shape == (0, 4)
    mu, cov = S.mean_and_cov(m, x)
    # sample covariance of n Gaussian draws (n − 1 in the denominator): Var S_ij = (Σ_ii Σ_jj + Σ_ij²)/(n − 1); the mean: Σ_ii/n
    se_cov = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / (n - 1))
    dev = np.abs(np.cov(s, rowvar=False) - cov) / se_cov
    print("sample covariance, deviations in standard errors:\n", dev)
    assert np.all(dev <= 5.0)
    assert np.all(np.abs(s.mean(axis=0) - mu) <= 5.0 * np.sqrt(np.diag(cov) / n))


def test_sample_joint_jitter_ladder(monkeypatch):
    sf2 = SF2
    tried = []
    real = np.linalg.cholesky

    def spy(a):
        tried.append(a[0, 0] - spy.base)                     # the jitter of this attempt (to the rounding of σ_f² + jitter)
        return real(a)

    m = _model(0.0)
    # a covariance with the eigenvalue −1e-9·σ_f²: the rungs 1e-12 … 1e-10 fail, 1e-9 leaves an exact zero pivot or a rounding-level one,
    # 1e-8 is positive definite
    c = sf2 * np.array([[1.0, 1.0 + 1e-9], [1.0 + 1e-9, 1.0]])
    monkeypatch.setattr(S, "mean_and_cov", lambda model, x: (np.zeros(2), c))
    spy.base = c[0, 0]
    monkeypatch.setattr(np.linalg, "cholesky", spy)
    s = abo.sample_joint(m, np.zeros((2, 2)), 7, rng=0)
    assert s.shape == (7, 2) and np.all(np.isfinite(s))
    rungs = np.array(tried) / sf2
    assert 4 <= len(rungs) <= 5
    np.testing.assert_allclose(rungs, [10.0 ** e for e in range(-12, -12 + len(rungs))], rtol=1e-3)
    # beyond the ladder: PosDefException once the 1e-6·σ_f² rung has failed, seven rungs tried
    tried.clear()
    bad = sf2 * np.array([[1.0, 1.001], [1.001, 1.0]])
    spy.base = bad[0, 0]
    monkeypatch.setattr(S, "mean_and_cov", lambda model, x: (np.zeros(2), bad))
    with pytest.raises(abo.PosDefException):
        abo.sample_joint(m, np.zeros((2, 2)), 3, rng=0)
    np.testing.assert_allclose(np.array(tried) / sf2, [10.0 ** e for e in range(-12, -5)], rtol=1e-3)
    # a given jitter is used alone
    tried.clear()
    with pytest.raises(abo.PosDefException):
        abo.sample_joint(m, np.zeros((2, 2)), 3, rng=0, jitter=1e-10)
    assert len(tried) == 1


def test_sample_joint_on_a_singular_covariance(monkeypatch):
    """duplicate points and a factor without noise, one of them a training point: the checker's covariance is singular (two equal
    rows, and a zero row up to rounding), the plain factorisation has nothing to stand on, and the ladder's first rungs deliver draws
    in which the duplicates agree to the jitter's scale"""
    monkeypatch.setattr(S, "mean_and_cov", _stub_mean_and_cov(0.0))
    X, _ = _problem()
    x = np.array([[0.4, 0.6], [0.4, 0.6], X[3], [0.9, 0.2]])
    _, cov = S.mean_and_cov(None, x)
    assert np.array_equal(cov[0], cov[1]) and np.linalg.eigvalsh(cov)[0] <= 1e-14 * SF2
    assert abs(cov[2, 2]) <= 1e-12 * SF2
    s = abo.sample_joint(_model(0.0), x, 500, rng=1)
    assert s.shape == (500, 4) and np.all(np.isfinite(s))
    assert np.max(np.abs(s[:, 0] - s[:, 1])) <= 10.0 * math.sqrt(2e-6 * SF2)
    assert np.std(s[:, 3]) > 0.0
