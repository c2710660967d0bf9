"""Leave-one-out cross-validation on the device: abo_loo (one pass over the triangle of L⁻ᵀ), abo_loo_grad (K⁻¹ and K⁻¹·∂K/∂log ℓ on the
fp64 MFMA GEMM, one pass over their rows) and the Python host on top of them.

The checker is tests/loo_oracle.py: its brute force (N refits on N − 1 points) is the reference for the values, its dense closed form
and central differences of its value for the gradient.  Problem as in tests/test_gpu_ard.py.  Shapes: every family over
N ∈ {1, 2, 16, 17, 128, 129, 300} at d = 3 (one point, a pair, the workgroup edges of the two row kernels, the 128-tile edge, a ragged last
tile with three tiles in the products), d ∈ {1, 8} at N = 129, and six duplicated points at N = 40.  Value errors are scaled
|Δμ|/max(1, |μ|), |Δσ²|/σ_f², |Δlpd|/max(1, |lpd|), |Δnlpl|/max(1, |nlpl|) and held under 1e-9 (the value-agreement bar of the NLML tests)
and under 100 × the error recorded on an MI355X in tests/golden/loo_bounds.json (floor 1e-13): tests.parity_record.check."""
import ctypes as C
import json
import math
import os
from functools import lru_cache

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import _lib, synth
from oracle import gp_oracle as O
from tests import loo_oracle as LO
from tests import parity_record
from tests.parity_record import check

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_bounds.json")) as _f:
    parity_record.BOUNDS.update(json.load(_f))             # every case here is named loo_*: nothing of parity_bounds.json is replaced

FAMS = {O.SE: abo.SqExponentialKernel, O.MATERN52: abo.Matern52Kernel, O.MATERN72: abo.ApproxMatern72Kernel, O.MATERN32: abo.Matern32Kernel}
SHAPES = [(N, 3) for N in (1, 2, 16, 17, 128, 129, 300)] + [(129, d) for d in (1, 8)]
CASES = [(f, N, d, False) for f in FAMS for (N, d) in SHAPES] + [(f, 40, 3, True) for f in FAMS]
SF2, NOISE, MEAN_C, ELL = 1.7, 1e-2, 0.3, 0.6
HARD = 1e-9


def problem(N, d, dup):
    X = synth.points(1, N, d)
    if dup:
        X[N // 2:N // 2 + 6] = X[:6]                        # six pairs at distance 0
    return X, synth.objective(X, 0.1) + 0.3


def model(family, ell=ELL, noise=NOISE, **kw):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(FAMS[family](), ell), noise, mean=abo.ConstMean(MEAN_C), **kw)


def loo_host(m):
    """abo_loo into host arrays → (mu, var, lpd, nlpl)"""
    n, d = C.c_int64(), C.c_int32()
    _lib.check(_lib.lib().abo_get_n(m._require(), C.byref(n), C.byref(d)))
    mu, var, lpd = (np.full(n.value, np.nan) for _ in range(3))
    v = C.c_double(float("nan"))
    _lib.check(_lib.lib().abo_loo(m._require(), mu.ctypes.data, var.ctypes.data, lpd.ctypes.data, C.byref(v), _lib.HOST))
    return mu, var, lpd, v.value


def loo_device(m, N):
    import torch
    mu, var, lpd = (torch.full((N,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3))
    v = C.c_double(float("nan"))
    _lib.check(_lib.lib().abo_loo(m._require(), mu.data_ptr(), var.data_ptr(), lpd.data_ptr(), C.byref(v), _lib.DEVICE))
    return mu.cpu().numpy(), var.cpu().numpy(), lpd.cpu().numpy(), v.value


def loo_grad(m):
    """abo_loo_grad → (nlpl, d_log_ell, d_log_sigma_f2, d_log_noise)"""
    o = [C.c_double(float("nan")) for _ in range(4)]
    _lib.check(_lib.lib().abo_loo_grad(m._require(), *(C.byref(x) for x in o)))
    return tuple(x.value for x in o)


def bits(*xs):
    return b"".join(np.asarray(x, dtype=np.float64).tobytes() for x in xs)


@lru_cache(maxsize=None)
def case(family, N, d, dup):
    """everything the tests of one case compare, computed once: both calls twice on one handle, the device-memory variant, and the
    checker's brute force, dense gradient and central differences"""
    X, y = problem(N, d, dup)
    m = abo.update(model(family), X, y)
    out = {"X": X, "y": y}
    out["loo"], out["grad"] = loo_host(m), loo_grad(m)
    out["loo_again"], out["grad_again"] = loo_host(m), loo_grad(m)
    out["loo_dev"] = loo_device(m, N)
    out["brute"] = LO.brute_force(family, ELL, SF2, NOISE, MEAN_C, X, y)
    out["ref_grad"] = LO.nlpl_and_grad(family, ELL, SF2, NOISE, MEAN_C, X, y)
    out["fd"] = LO.central_differences(family, ELL, SF2, NOISE, MEAN_C, X, y, h=1e-5)
    return out


def name_of(family, N, d, dup):
    return f"loo_fam{family}_N{N}_d{d}" + ("_dup" if dup else "")


def value_errors(got, ref):
    mu, var, lpd, v = got
    rmu, rvar, rlpd, rv = ref
    return {"mu": float(np.max(np.abs(mu - rmu) / np.maximum(1.0, np.abs(rmu)))), "var": float(np.max(np.abs(var - rvar))) / SF2,
            "lpd": float(np.max(np.abs(lpd - rlpd) / np.maximum(1.0, np.abs(rlpd)))), "nlpl": abs(v - rv) / max(1.0, abs(rv))}


@pytest.mark.parametrize("family,N,d,dup", CASES)
def test_values_against_brute_force(family, N, d, dup):
    c = case(family, N, d, dup)
    errs = value_errors(c["loo"], c["brute"])
    print(name_of(family, N, d, dup), errs)
    for k, e in errs.items():
        check(name_of(family, N, d, dup), k, e, HARD)


@pytest.mark.parametrize("family,N,d,dup", CASES)
def test_gradient_against_central_differences_and_the_dense_closed_form(family, N, d, dup):
    """the bars of test_nlml_gradient_against_oracle_finite_differences: h = 1e-5, rtol 2e-6, atol 1e-6·max(1, |v|)"""
    c = case(family, N, d, dup)
    v, g = c["grad"][0], np.array(c["grad"][1:])
    atol = 1e-6 * max(1.0, abs(v))
    print(name_of(family, N, d, dup), "device", g, "closed form", c["ref_grad"][1:], "central differences", c["fd"])
    np.testing.assert_allclose(g, c["fd"], rtol=2e-6, atol=atol)
    np.testing.assert_allclose(g, c["ref_grad"][1:], rtol=2e-6, atol=atol)
    assert abs(v - c["ref_grad"][0]) <= HARD * max(1.0, abs(v))


@pytest.mark.parametrize("family,N,d,dup", CASES)
def test_bits(family, N, d, dup):
    """two calls return the same bytes, abo_loo_grad's nlpl is abo_loo's, device output equals host output"""
    c = case(family, N, d, dup)
    assert bits(*c["loo"]) == bits(*c["loo_again"]) and bits(*c["grad"]) == bits(*c["grad_again"])
    assert bits(c["grad"][0]) == bits(c["loo"][3])
    assert bits(*c["loo"]) == bits(*c["loo_dev"])
    assert not np.isnan(bits_as_array(c["loo"])).any()


def bits_as_array(t):
    return np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in t])


@pytest.mark.parametrize("family", list(FAMS))
def test_zero_noise_has_zero_noise_partial(family):
    """a factor built without noise: d_log_noise is exactly 0, the other two partials still follow the checker (N = 17, ℓ = 0.2)"""
    X, y = problem(17, 3, False)
    m = abo.update(model(family, ell=0.2, noise=0.0), X, y)
    v, g_ell, g_sf2, g_noise = loo_grad(m)
    assert g_noise == 0.0
    rv, r_ell, r_sf2, _ = LO.nlpl_and_grad(family, 0.2, SF2, 0.0, MEAN_C, X, y)
    fd_ell, fd_sf2, _ = LO.central_differences(family, 0.2, SF2, 0.0, MEAN_C, X, y, h=1e-5)
    atol = 1e-6 * max(1.0, abs(v))
    np.testing.assert_allclose([g_ell, g_sf2], [fd_ell, fd_sf2], rtol=2e-6, atol=atol)
    np.testing.assert_allclose([g_ell, g_sf2], [r_ell, r_sf2], rtol=2e-6, atol=atol)


def test_views_stop_at_their_own_rows():
    """126 points + 4 appended: the view crosses the tile edge; the parent keeps its values bit for bit; the gradient refuses the view"""
    X, y = problem(130, 3, False)
    parent = abo.update(model(O.MATERN52, n_max=256), X[:126], y[:126])
    before = loo_host(parent)
    view = parent
    for i in range(126, 130):
        view = abo.append(view, X[i], float(y[i]))
    errs = value_errors(loo_host(view), LO.brute_force(O.MATERN52, ELL, SF2, NOISE, MEAN_C, X, y))
    print("loo_view_130", errs)
    for k, e in errs.items():
        check("loo_view_130", k, e, HARD)
    errs = value_errors(before, LO.brute_force(O.MATERN52, ELL, SF2, NOISE, MEAN_C, X[:126], y[:126]))
    for k, e in errs.items():
        check("loo_view_parent_126", k, e, HARD)
    assert bits(*loo_host(parent)) == bits(*before)
    L = _lib.lib()
    v = C.c_double()
    assert L.abo_loo_grad(view._require(), C.byref(v), None, None, None) == _lib.ABO_EINVAL
    assert "freshly fitted" in _lib.last_error()
    assert L.abo_loo_grad(parent._require(), C.byref(v), None, None, None) == _lib.ABO_EINVAL       # a longer view lives on its storage


def test_arguments():
    L = _lib.lib()
    X, y = problem(30, 3, False)
    gp = model(O.MATERN52)
    m = abo.update(gp, X, y)
    v, w = C.c_double(), C.c_double()
    # every output NULL, and any single one
    assert L.abo_loo(m._require(), None, None, None, None, _lib.HOST) == _lib.ABO_OK
    assert L.abo_loo(m._require(), None, None, None, None, _lib.DEVICE) == _lib.ABO_OK
    assert L.abo_loo_grad(m._require(), None, None, None, None) == _lib.ABO_OK
    assert L.abo_loo(m._require(), None, None, None, C.byref(v), _lib.HOST) == _lib.ABO_OK
    assert L.abo_loo_grad(m._require(), None, None, C.byref(w), None) == _lib.ABO_OK
    ref = loo_host(m)
    assert bits(v.value) == bits(ref[3]) and bits(w.value) == bits(loo_grad(m)[2])
    var = np.empty(30)
    assert L.abo_loo(m._require(), None, var.ctypes.data, None, None, _lib.HOST) == _lib.ABO_OK and bits(var) == bits(ref[1])
    assert L.abo_loo(m._require(), None, None, None, C.byref(v), 2) == _lib.ABO_EINVAL
    # null handle
    assert L.abo_loo(None, None, None, None, C.byref(v), _lib.HOST) == _lib.ABO_EINVAL
    assert L.abo_loo_grad(None, C.byref(v), None, None, None) == _lib.ABO_EINVAL
    # not fitted
    hp, prm = C.c_void_p(), gp._params()
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    try:
        assert L.abo_loo(hp, None, None, None, C.byref(v), _lib.HOST) == _lib.ABO_EINVAL
        assert "not conditioned" in _lib.last_error()
        assert L.abo_loo_grad(hp, C.byref(v), None, None, None) == _lib.ABO_EINVAL
    finally:
        L.abo_destroy(hp)
    # a gradient-enhanced handle
    Xg = synth.points(1, 12, 2)
    Yg = np.column_stack([np.sin(Xg).sum(1), np.cos(Xg)])
    mg = abo.update(abo.GradientGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.7), 3, 1e-3), Xg, Yg)
    assert L.abo_loo(mg._require(), None, None, None, C.byref(v), _lib.HOST) == _lib.ABO_EINVAL
    assert L.abo_loo_grad(mg._require(), C.byref(v), None, None, None) == _lib.ABO_EINVAL


def test_python_leave_one_out_on_an_ard_model():
    """no coordinates cross the call: the ARD model's values are those of the isotropic model fitted on hand-scaled data"""
    ells = np.array([0.3, 1.7, 0.08, 6.0])
    X, y = synth.standardized_problem(60, 4, 0.02)
    X = X * np.array([1.0, 4.0, 0.2, 10.0])
    kern = lambda ell: 1.3 * abo.with_lengthscale(abo.Matern52Kernel(), ell)
    ard = abo.update(abo.HipStandardGP(kern(ells), 1e-3), X, y)
    hand = abo.update(abo.HipStandardGP(kern(1.0), 1e-3), X / ells, y)
    a, h = abo.leave_one_out(ard), abo.leave_one_out(hand)
    assert all(isinstance(x, np.ndarray) and x.shape == (60,) for x in a[:3]) and isinstance(a[3], float)
    assert bits(*a) == bits(*h)
    errs = value_errors(a, LO.brute_force(O.MATERN52, 1.0, 1.3, 1e-3, 0.0, X / ells, y))
    for k, e in errs.items():
        check("loo_python_ard_60", k, e, HARD)


def test_python_loo_search_goes_downhill_and_the_default_is_the_nlml_search():
    from scipy.optimize import minimize
    X, y = synth.standardized_problem(64, 3, 0.3)
    m = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 2.0), 0.09)
    start = [math.log(2.0), 0.0]
    out = abo.optimize_hyperparameters(m, X, y, start, objective="loo", rng=np.random.default_rng(0))
    assert out is not m and out.gpx is None
    p = [math.log(abo.get_lengthscale(out)[0]), math.log(abo.get_scale(out)[0])]
    v0, v1 = abo.loo_and_grad(m, start, X, y)[0], abo.loo_and_grad(out, p, X, y)[0]
    print("nlpl at the start", v0, "at the end", v1, "parameters", p)
    assert v1 < v0
    # the value and gradient the search ran on are the checker's
    v, g = abo.loo_and_grad(m, start, X, y)
    rv, r_ell, r_sf2, _ = LO.nlpl_and_grad(O.MATERN52, 2.0, 1.0, 0.09, 0.0, X, y)
    assert abs(v - rv) <= HARD * max(1.0, abs(rv))
    np.testing.assert_allclose(g, [r_ell, r_sf2], rtol=2e-6, atol=1e-6 * max(1.0, abs(rv)))
    # without the keyword: the NLML search as it always ran — SciPy on nlml_and_grad with the same box, start and options
    plain = abo.optimize_hyperparameters(m, X, y, start, rng=np.random.default_rng(0))
    named = abo.optimize_hyperparameters(m, X, y, start, rng=np.random.default_rng(0), objective="nlml")
    lower, upper = np.log([1e-3, 1e-3]), np.log([1e3, 1e6])
    eps2 = 2 * np.finfo(np.float64).eps
    res = minimize(lambda q: abo.nlml_and_grad(m, [q[0], q[1]], X, y), np.clip(np.array(start), lower + eps2, upper - eps2), jac=True,
                   method="L-BFGS-B", bounds=list(zip(lower, upper)), options={"gtol": 1e-6, "ftol": 2.2e-9, "maxls": 20})
    assert res.success
    for got in (plain, named):
        assert abo.get_lengthscale(got) == [math.exp(res.x[0])] and abo.get_scale(got) == [math.exp(res.x[1])]
