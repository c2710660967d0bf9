"""Joint posterior covariance between point sets on the device: abo_predict_cov and the Python host on top of it.

The checker is tests/cov_oracle.py (K = σ_f²κ + σ²I, cho_factor / cho_solve, cov = K_ab − K_aX K⁻¹ K_Xb).  Shapes, the smallest that
cross every boundary: N = 200 at d = 3 (two 128-tiles, the second ragged) and N = 128 at d = 1 (one exact tile), Ma = 130 against
Mb = 257 (ragged, two against three tiles) plus Ma = 1, every kernel family, σ² = 1e-2 and σ² = 0 on a model built with the opt-in
jitter (ℓ = 0.2 there, so that K stays well conditioned: κ₂(K) ≤ 4e5 for every family; the noise the factor was really built with is
read off L₀₀ and handed to the checker, whichever rung of the ladder ran).

Errors are max|cov_gpu − cov_oracle|/σ_f² (means: |Δμ|/max(1, |μ|)), held under the project's 1e-6 bar and under 100 × the error
recorded on an MI355X in tests/golden/cov_bounds.json (floor 1e-13): tests.parity_record.check.  The record is a file of its own, as
leave-one-out's is: tests/golden/parity_bounds.json is an existing yardstick and stays as it is."""
import ctypes as C
import json
import os
from functools import lru_cache

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import _lib, synth
from oracle import gp_oracle as O
from tests import cov_oracle as CO
from tests import parity_record
from tests.parity_record import check

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cov_bounds.json")) as _f:
    parity_record.BOUNDS.update(json.load(_f))             # every case here is named cov_*: nothing of parity_bounds.json is replaced

FAMS = {O.SE: abo.SqExponentialKernel, O.MATERN52: abo.Matern52Kernel, O.MATERN72: abo.ApproxMatern72Kernel, O.MATERN32: abo.Matern32Kernel}
SF2, MEAN_C, JITTER = 1.7, 0.3, 1e-8
MA, MB = 130, 257
HARD = 1e-6
#         N,   d, noise, ell
CONFIGS = [(200, 3, 1e-2, 0.6), (128, 1, 1e-2, 0.6), (200, 3, 0.0, 0.2)]
CASES = [(f, *c) for f in FAMS for c in CONFIGS]


def problem(N, d):
    X = synth.points(1, N, d)
    return X, synth.objective(X, 0.1) + 0.3


def queries(d):
    """Za (130) and Zb (257) in [−0.1, 1.1]^d: inside and outside the data; Zb's first three points are points of Za"""
    rng = np.random.default_rng(17)
    za, zb = rng.random((MA, d)) * 1.2 - 0.1, rng.random((MB, d)) * 1.2 - 0.1
    zb[:3] = za[:3]
    return za, zb


def model(family, ell, noise, **kw):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(FAMS[family](), ell), noise, mean=abo.ConstMean(MEAN_C),
                             jitter=(JITTER if noise == 0.0 else 0.0), n_max=256, **kw)


def predict_cov(m, za, zb=None, want_mu=True, mb_arg=None):
    """abo_predict_cov on host arrays → (status, mu_a, mu_b, cov), every output pre-filled with NaN"""
    za = np.ascontiguousarray(za, dtype=np.float64)
    ma, d = za.shape
    mb = ma if zb is None else zb.shape[0]
    zb = None if zb is None else np.ascontiguousarray(zb, dtype=np.float64)
    mu_a = np.full(ma, np.nan) if want_mu else None
    mu_b = np.full(mb, np.nan) if (want_mu and zb is not None) else None
    cov = np.full((ma, mb), np.nan)
    st = _lib.lib().abo_predict_cov(m._require(), za.ctypes.data, ma, None if zb is None else zb.ctypes.data,
                                    (0 if zb is None else mb) if mb_arg is None else mb_arg, d, _lib.HOST,
                                    None if mu_a is None else mu_a.ctypes.data, None if mu_b is None else mu_b.ctypes.data, cov.ctypes.data, _lib.HOST)
    return st, mu_a, mu_b, cov


def ok(r):
    _lib.check(r[0])
    return r[1:]


def noise_used(m, noise):
    """the noise the factor was built with: noise itself, or — a model with the opt-in jitter — the rung of noise + jitter·10^r nearest to
    L₀₀² − σ_f² (L₀₀² = k(x₀, x₀) + that noise)"""
    if noise != 0.0:
        return noise
    L00 = abo.get_factor(m)[0][0, 0]
    rungs = np.array([0.0] + [JITTER * 10.0 ** r for r in range(4)])
    return float(rungs[np.argmin(np.abs(rungs - (L00 * L00 - SF2)))])


def bits(*xs):
    return b"".join(np.ascontiguousarray(x, dtype=np.float64).tobytes() for x in xs)


@lru_cache(maxsize=None)
def case(family, N, d, noise, ell):
    """everything the tests of one case compare, computed once and left unchanged"""
    X, y = problem(N, d)
    za, zb = queries(d)
    m = abo.update(model(family, ell, noise), X, y)
    out = {"X": X, "y": y, "za": za, "zb": zb, "m": m}
    out["rect"] = ok(predict_cov(m, za, zb))
    out["sym"] = ok(predict_cov(m, za))
    out["rect_again"], out["sym_again"] = ok(predict_cov(m, za, zb)), ok(predict_cov(m, za))
    out["rect_aa"] = ok(predict_cov(m, za, za))
    out["one_sym"], out["one_rect"] = ok(predict_cov(m, za[:1])), ok(predict_cov(m, za[:1], zb))
    out["mu_a"], out["var_a"] = abo.mean_and_var(m, za)
    out["mu_b"] = abo.posterior_mean(m, zb)
    nu = noise_used(m, noise)
    out["ref_rect"] = CO.posterior_cov(family, ell, SF2, nu, X, za, zb)
    out["ref_mu"], out["ref_sym"] = CO.mean_and_cov(family, ell, SF2, nu, MEAN_C, X, y, za)
    return out


def name_of(family, N, d, noise, ell):
    return f"cov_fam{family}_N{N}_d{d}" + ("_nonoise" if noise == 0.0 else "")


def err(a, b):
    return float(np.max(np.abs(a - b))) / SF2


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_parity_with_the_oracle(family, N, d, noise, ell):
    c = case(family, N, d, noise, ell)
    nm = name_of(family, N, d, noise, ell)
    errs = {"rect": err(c["rect"][2], c["ref_rect"]), "sym": err(c["sym"][2], c["ref_sym"]),
            "one_sym": err(c["one_sym"][2], c["ref_sym"][:1, :1]), "one_rect": err(c["one_rect"][2], c["ref_rect"][:1]),
            "mu": float(np.max(np.abs(c["sym"][0] - c["ref_mu"]) / np.maximum(1.0, np.abs(c["ref_mu"]))))}
    print(nm, errs)
    for r in ("rect", "sym", "one_sym", "one_rect"):
        assert np.all(np.isfinite(c[r][2]))
    for k, e in errs.items():
        check(nm, k, e, HARD)


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_symmetric_form(family, N, d, noise, ell):
    """symmetric bit for bit; its diagonal is abo_predict's variance and its lower triangle the rectangular call's with Zb = Za — other
    summation orders, so to rounding: through the same record"""
    c = case(family, N, d, noise, ell)
    nm = name_of(family, N, d, noise, ell)
    cov = c["sym"][2]
    assert bits(cov) == bits(cov.T)
    e_diag = err(np.diag(cov), c["var_a"])
    lo = np.tril_indices(MA)
    e_rect = err(cov[lo], c["rect_aa"][2][lo])
    print(nm, {"diag_vs_predict": e_diag, "sym_vs_rect": e_rect})
    check(nm, "diag_vs_predict", e_diag, HARD)
    check(nm, "sym_vs_rect", e_rect, HARD)
    assert c["one_sym"][2].shape == (1, 1)
    check(nm, "one_vs_predict", abs(c["one_sym"][2][0, 0] - c["var_a"][0]) / SF2, HARD)


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_positive_semidefinite_to_the_measured_error(family, N, d, noise, ell):
    """Weyl: |λ_min(A) − λ_min(B)| ≤ ‖A − B‖₂ ≤ Ma·max|A − B| — the bound is the measured error, no free constant"""
    c = case(family, N, d, noise, ell)
    cov, ref = c["sym"][2], c["ref_sym"]
    lam, lam_ref = np.linalg.eigvalsh(cov)[0], np.linalg.eigvalsh(ref)[0]
    slack = MA * float(np.max(np.abs(cov - ref)))
    print(name_of(family, N, d, noise, ell), {"lambda_min": lam, "lambda_min_oracle": lam_ref, "slack": slack})
    assert lam >= lam_ref - slack


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_means_and_determinism(family, N, d, noise, ell):
    """mu_a / mu_b are abo_predict's bits in both forms; two calls return identical bits"""
    c = case(family, N, d, noise, ell)
    assert bits(c["rect"][0]) == bits(c["mu_a"]) and bits(c["rect"][1]) == bits(c["mu_b"])
    assert bits(c["sym"][0]) == bits(c["mu_a"]) and c["sym"][1] is None
    assert bits(c["one_rect"][0]) == bits(c["mu_a"][:1]) and bits(c["one_rect"][1]) == bits(c["mu_b"])
    assert bits(*c["rect"]) == bits(*c["rect_again"])
    assert bits(c["sym"][0], c["sym"][2]) == bits(c["sym_again"][0], c["sym_again"][2])


@pytest.mark.parametrize("family", list(FAMS))
def test_device_space_equals_host_space(family):
    import torch
    N, d, noise, ell = CONFIGS[0]
    c = case(family, N, d, noise, ell)
    m = c["m"]
    za, zb = torch.from_numpy(c["za"]).cuda(), torch.from_numpy(c["zb"]).cuda()
    mu_a, mu_b = (torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for n in (MA, MB))
    cov = torch.full((MA, MB), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().abo_predict_cov(m._require(), za.data_ptr(), MA, zb.data_ptr(), MB, d, _lib.DEVICE, mu_a.data_ptr(), mu_b.data_ptr(),
                                          cov.data_ptr(), _lib.DEVICE))
    assert bits(mu_a.cpu().numpy(), mu_b.cpu().numpy(), cov.cpu().numpy()) == bits(*c["rect"])
    # and through the Python host: tensors in, tensors out
    pc = abo.posterior_cov(m, za)
    assert pc.is_cuda and bits(pc.cpu().numpy()) == bits(c["sym"][2])
    mu, pc2 = abo.mean_and_cov(m, c["za"])
    assert isinstance(pc2, np.ndarray) and bits(mu, pc2) == bits(c["sym"][0], c["sym"][2])
    assert bits(abo.posterior_cov(m, c["za"], c["zb"])) == bits(c["rect"][2])
    # cov alone, and the means alone
    assert bits(ok(predict_cov(m, c["za"], c["zb"], want_mu=False))[2]) == bits(c["rect"][2])
    mu_only = np.full(MA, np.nan)
    _lib.check(_lib.lib().abo_predict_cov(m._require(), c["za"].ctypes.data, MA, None, MA, d, _lib.HOST, mu_only.ctypes.data, None, None, _lib.HOST))
    assert bits(mu_only) == bits(c["mu_a"])


@pytest.mark.parametrize("family", list(FAMS))
def test_views(family):
    """a parent returns the same bits before and after a child was appended in place (row 200 of the shared factor then holds the
    child's branch); the child agrees with the checker refitted on 201 points"""
    N, d, noise, ell = CONFIGS[0]
    c = case(family, N, d, noise, ell)
    X, y, za, zb = c["X"], c["y"], c["za"], c["zb"]
    m = abo.update(model(family, ell, noise), X, y)
    before_r, before_s = ok(predict_cov(m, za, zb)), ok(predict_cov(m, za))
    assert bits(*before_r) == bits(*c["rect"])
    xs, ys = np.array([0.37, 0.52, 0.81]), 0.9
    m2 = abo.append(m, xs, ys)
    after_r, after_s = ok(predict_cov(m, za, zb)), ok(predict_cov(m, za))
    assert bits(*before_r) == bits(*after_r)
    assert bits(before_s[0], before_s[2]) == bits(after_s[0], after_s[2])
    X2, y2 = np.vstack([X, xs[None, :]]), np.append(y, ys)
    child_r, child_s = ok(predict_cov(m2, za, zb)), ok(predict_cov(m2, za))
    nm = f"cov_fam{family}_view201"
    e = {"rect": err(child_r[2], CO.posterior_cov(family, ell, SF2, noise, X2, za, zb)),
         "sym": err(child_s[2], CO.posterior_cov(family, ell, SF2, noise, X2, za))}
    print(nm, e)
    for k, v in e.items():
        check(nm, k, v, HARD)
    assert bits(child_s[2]) == bits(child_s[2].T)
    assert bits(child_r[0]) == bits(abo.posterior_mean(m2, za))
    # the parent once more, after the child has run its own call on the shared storage
    assert bits(*ok(predict_cov(m, za, zb))) == bits(*before_r)


@pytest.mark.parametrize("family", [O.SE, O.MATERN52])
def test_engine_setting_changes_nothing(family):
    N, d, noise, ell = CONFIGS[0]
    c = case(family, N, d, noise, ell)
    for eng in ("fp64", "int8"):
        m = abo.update(model(family, ell, noise, contraction=eng), c["X"], c["y"])
        abo.posterior_var(m, c["za"])                           # the handle's own engine has run (and built its state) first
        assert bits(*ok(predict_cov(m, c["za"], c["zb"]))) == bits(*c["rect"]), eng
        r = ok(predict_cov(m, c["za"]))
        assert bits(r[0], r[2]) == bits(c["sym"][0], c["sym"][2]), eng


def test_ard_model_equals_the_hand_scaled_isotropic_one():
    X, y = problem(200, 3)
    za, zb = queries(3)
    ell = np.array([0.5, 0.7, 0.9])
    ard = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), list(ell)), 1e-2, mean=abo.ConstMean(MEAN_C)), X, y)
    iso = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), 1.0), 1e-2, mean=abo.ConstMean(MEAN_C)), X / ell, y)
    assert bits(abo.posterior_cov(ard, za, zb)) == bits(abo.posterior_cov(iso, za / ell, zb / ell))
    a, b = abo.mean_and_cov(ard, za), abo.mean_and_cov(iso, za / ell)
    assert bits(*a) == bits(*b)
    with pytest.raises(abo.DimensionMismatch):
        abo.posterior_cov(ard, za[:, :2])


def last_error_after(st):
    assert st == _lib.ABO_EINVAL
    text = _lib.last_error()
    assert text.strip()
    return text


def test_refusals():
    """ABO_EINVAL and a text in abo_last_error; the outputs stay untouched (nothing was launched or copied)"""
    N, d, noise, ell = CONFIGS[0]
    c = case(O.MATERN52, N, d, noise, ell)
    m, za, zb = c["m"], c["za"], c["zb"]
    L = _lib.lib()
    cov = np.full((MA, MA), np.nan)
    mu = np.full(MA, np.nan)
    # Ma = 0, Ma = 8193
    for ma in (0, 8193):
        big = np.zeros((max(ma, 1), d))
        assert "Ma" in last_error_after(L.abo_predict_cov(m._require(), big.ctypes.data, ma, None, 0, d, _lib.HOST, None, None, cov.ctypes.data, _lib.HOST))
    assert "Mb" in last_error_after(L.abo_predict_cov(m._require(), za.ctypes.data, MA, zb.ctypes.data, 8193, d, _lib.HOST, None, None, cov.ctypes.data, _lib.HOST))
    # mu_b with Zb = NULL; Mb that is neither 0 nor Ma
    assert "mu_b" in last_error_after(L.abo_predict_cov(m._require(), za.ctypes.data, MA, None, 0, d, _lib.HOST, None, mu.ctypes.data, cov.ctypes.data, _lib.HOST))
    assert "Mb" in last_error_after(L.abo_predict_cov(m._require(), za.ctypes.data, MA, None, MA - 1, d, _lib.HOST, None, None, cov.ctypes.data, _lib.HOST))
    # an unfitted handle
    hp = C.c_void_p()
    prm = model(O.MATERN52, ell, noise)._params()
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    try:
        assert "not conditioned" in last_error_after(L.abo_predict_cov(hp.value, za.ctypes.data, MA, None, 0, d, _lib.HOST, mu.ctypes.data, None, cov.ctypes.data, _lib.HOST))
    finally:
        L.abo_destroy(hp.value)
    # a gradient-enhanced handle
    Xg = synth.points(2, 20, d)
    g = abo.update(abo.HipGradientGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.6), d + 1, 1e-2), Xg, np.zeros((20, d + 1)))
    assert "gradient" in last_error_after(L.abo_predict_cov(g._require(), za.ctypes.data, MA, None, 0, d, _lib.HOST, mu.ctypes.data, None, cov.ctypes.data, _lib.HOST))
    with pytest.raises(TypeError, match="gradient"):
        abo.posterior_cov(g, za)
    # the wrong dimension: ABO_EDIM from the library, DimensionMismatch from the host
    assert L.abo_predict_cov(m._require(), za.ctypes.data, MA, None, 0, d - 1, _lib.HOST, None, None, cov.ctypes.data, _lib.HOST) == _lib.ABO_EDIM
    with pytest.raises(abo.DimensionMismatch):
        abo.posterior_cov(m, za[:, :2])
    assert np.all(np.isnan(cov)) and np.all(np.isnan(mu))
    # the handle still serves
    assert bits(ok(predict_cov(m, za))[2]) == bits(c["sym"][2])


def test_sample_joint_on_the_device_covariance():
    """exact joint draws at M = 4 points from the device's (mu, cov): seeded, and their first two moments within 5 standard errors of the
    checker's (Var S_ij = (Σ_ii Σ_jj + Σ_ij²)/(n − 1))"""
    N, d, noise, ell = CONFIGS[0]
    c = case(O.MATERN52, N, d, noise, ell)
    x, n = c["za"][:4], 20000
    s = abo.sample_joint(c["m"], x, n, rng=np.random.default_rng(2))
    assert s.shape == (n, 4) and bits(s) == bits(abo.sample_joint(c["m"], x, n, rng=np.random.default_rng(2)))
    mu, cov = c["ref_mu"][:4], c["ref_sym"][:4, :4]
    se = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / (n - 1))
    assert np.all(np.abs(np.cov(s, rowvar=False) - cov) <= 5.0 * se)
    assert np.all(np.abs(s.mean(axis=0) - mu) <= 5.0 * np.sqrt(np.diag(cov) / n))
