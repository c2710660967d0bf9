"""ARD length scales on the device: abo_nlml_grad_ard (the per-coordinate trace sweep) and the Python host's ARD models.

The checker is tests/ard_oracle.py (the CPU oracle on scaled inputs; the analytic gradient densely).  Shapes: every family over
N ∈ {1, 16, 17, 128, 129, 300} at d = 3 (one point, the 16-row workgroup edge, the 128-tile edge where the weight switches, a ragged
last tile) and over d ∈ {1, 3, 5, 8, 16, 32} at N = 129 (d = 3 and 5 run with padded coordinates), plus one case with duplicated
training points (d2 = 0 off the diagonal).  Errors against the checker and against abo_nlml_grad are scaled by max(1, |nlml|) and held
under 1e-9 (the value-agreement bar of test_nlml_gradient_against_oracle_finite_differences) and under 100 × the error recorded on an
MI355X in tests/golden/ard_bounds.json (floor 1e-13): tests.parity_record.check with that file's values."""
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
from tests import ard_oracle as A
from tests import parity_record
from tests.parity_record import check

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ard_bounds.json")) as _f:
    parity_record.BOUNDS.update(json.load(_f))             # every case here is named ard_*: nothing of parity_bounds.json is replaced

FAMS = {O.SE: abo.SqExponentialKernel, O.MATERN52: abo.Matern52Kernel, O.MATERN72: abo.ApproxMatern72Kernel, O.MATERN32: abo.Matern32Kernel}
SHAPES = [(N, 3) for N in (1, 16, 17, 128, 129, 300)] + [(129, d) for d in (1, 5, 8, 16, 32)]
CASES = [(f, N, d, False) for f in FAMS for (N, d) in SHAPES] + [(f, 40, 3, True) for f in FAMS]
SF2, NOISE, MEAN_C, ELL_ISO = 1.7, 1e-2, 0.3, 0.6
HARD = 1e-9


def ells_for(d):
    """two decades, 0.1 … 10, in an order that is not monotone in the coordinate"""
    if d == 1:
        return np.array([0.6])
    return np.logspace(-1.0, 1.0, d)[np.random.default_rng(d).permutation(d)]


def problem(N, d, dup):
    X = synth.points(1, N, d)
    if dup:
        X[N // 2:N // 2 + 6] = X[:6]                        # six pairs at distance 0
    return X, synth.objective(X, 0.1) + 0.3


def grad_ard(model, d=None):
    """abo_nlml_grad_ard on the model's handle → (nlml, d_log_ell (d,), d_log_sigma_f2, d_log_noise)"""
    n, dm = C.c_int64(), C.c_int32()
    _lib.check(_lib.lib().abo_get_n(model._require(), C.byref(n), C.byref(dm)))
    d = dm.value if d is None else d
    v, s, z = C.c_double(), C.c_double(), C.c_double()
    g = (C.c_double * d)()
    _lib.check(_lib.lib().abo_nlml_grad_ard(model._require(), d, C.byref(v), g, C.byref(s), C.byref(z)))
    return v.value, np.array(list(g)), s.value, z.value


def grad_iso(model):
    v, g, s = C.c_double(), C.c_double(), C.c_double()
    _lib.check(_lib.lib().abo_nlml_grad(model._require(), C.byref(v), C.byref(g), C.byref(s)))
    return v.value, g.value, s.value


def bits(*xs):
    return b"".join(np.asarray(x, dtype=np.float64).tobytes() for x in xs)


@lru_cache(maxsize=None)
def case(family, N, d, dup):
    """everything the tests of one case compare, computed once: an isotropic handle (ℓ = 0.6, raw points) and an ARD handle (ℓ = 1 on
    pre-scaled points, through the Python model), each with both gradient calls, and the checker's values for both"""
    X, y = problem(N, d, dup)
    ells = ells_for(d)
    iso = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(FAMS[family](), ELL_ISO), NOISE, mean=abo.ConstMean(MEAN_C)), X, y)
    ard = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(FAMS[family](), ells), NOISE, mean=abo.ConstMean(MEAN_C)), X, y)
    out = {"X": X, "y": y, "ells": ells}
    for name, m, le in (("iso", iso, np.full(d, ELL_ISO)), ("ard", ard, ells)):
        first = grad_ard(m)
        out[name] = {"ard": first, "again": grad_ard(m), "iso": grad_iso(m), "ref": A.nlml_and_grad(family, le, SF2, NOISE, MEAN_C, X, y),
                     "ells": le}
    return out


def name_of(family, N, d, dup):
    return f"ard_fam{family}_N{N}_d{d}" + ("_dup" if dup else "")


@pytest.mark.parametrize("family,N,d,dup", CASES)
def test_sum_identity_and_shared_scalars(family, N, d, dup):
    """Σ_c d_log_ell[c] = abo_nlml_grad's d_log_ell on the same handle (ℓ = 0.6 and ℓ = 1); nlml and d_log_sigma_f2 bit for bit"""
    c = case(family, N, d, dup)
    for which in ("iso", "ard"):
        v, g, s, _ = c[which]["ard"]
        v0, g0, s0 = c[which]["iso"]
        assert bits(v, s) == bits(v0, s0)
        err = abs(g.sum() - g0) / max(1.0, abs(v))
        print(name_of(family, N, d, dup), which, "sum identity", err)
        check(name_of(family, N, d, dup), f"sum_{which}", err, HARD)


@pytest.mark.parametrize("family,N,d,dup", CASES)
def test_parity_with_the_analytic_gradient(family, N, d, dup):
    """d_log_ell, d_log_noise (and the shared scalars) against the checker's dense analytic values; the ARD handle's length scales
    spread over two decades, applied by pre-scaling"""
    c = case(family, N, d, dup)
    for which in ("iso", "ard"):
        v, g, s, z = c[which]["ard"]
        rv, rg, rs, rz = c[which]["ref"]
        scale = max(1.0, abs(rv))
        errs = {"nlml": abs(v - rv) / scale, "ell": float(np.max(np.abs(g - rg))) / scale, "sf2": abs(s - rs) / scale,
                "noise": abs(z - rz) / scale}
        print(name_of(family, N, d, dup), which, errs)
        for k, e in errs.items():
            check(name_of(family, N, d, dup), f"{k}_{which}", e, HARD)


@pytest.mark.parametrize("family,N,d,dup", CASES)
def test_against_central_differences_of_the_oracle(family, N, d, dup):
    """each ∂/∂log ℓ_c and ∂/∂log σ² against central differences of the CPU oracle's NLML: h = 1e-5, rtol 2e-6, atol 1e-6·max(1, |v|)"""
    c = case(family, N, d, dup)
    v, g, s, z = c["ard"]["ard"]
    fd_ell, fd_sf2, fd_noise = A.central_differences(family, c["ells"], SF2, NOISE, MEAN_C, c["X"], c["y"], h=1e-5)
    atol = 1e-6 * max(1.0, abs(v))
    np.testing.assert_allclose(g, fd_ell, rtol=2e-6, atol=atol)
    np.testing.assert_allclose([s, z], [fd_sf2, fd_noise], rtol=2e-6, atol=atol)


@pytest.mark.parametrize("family,N,d,dup", CASES)
def test_two_calls_return_the_same_bits(family, N, d, dup):
    c = case(family, N, d, dup)
    for which in ("iso", "ard"):
        assert bits(*c[which]["ard"]) == bits(*c[which]["again"])


def test_padded_coordinates_and_zero_noise():
    """d_log_noise is 0 when the factor was built without noise; a coordinate in which all points agree has partial exactly 0"""
    X = synth.points(1, 50, 3)
    X[:, 1] = 0.25
    y = synth.objective(X, 0.1)
    m = abo.update(abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.2), 0.0), X, y)
    v, g, s, z = grad_ard(m)
    assert z == 0.0 and g[1] == 0.0 and g[0] != 0.0 and g[2] != 0.0


def test_errors_and_null_outputs():
    L = _lib.lib()
    X, y = problem(30, 3, False)
    gp = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.5), 1e-2, n_max=64)
    m = abo.update(gp, X, y)
    v = C.c_double()
    g = (C.c_double * 40)()
    # NULL outputs are accepted, singly and all at once
    assert L.abo_nlml_grad_ard(m._require(), 3, None, None, None, None) == _lib.ABO_OK
    assert L.abo_nlml_grad_ard(m._require(), 3, C.byref(v), None, None, None) == _lib.ABO_OK and v.value == abo.nlml_fitted(m)
    assert L.abo_nlml_grad_ard(m._require(), 3, None, g, None, None) == _lib.ABO_OK
    # wrong d, d > 32 (also on a model that has d = 33), null handle
    assert L.abo_nlml_grad_ard(m._require(), 4, C.byref(v), g, None, None) == _lib.ABO_EDIM
    assert L.abo_nlml_grad_ard(m._require(), 33, C.byref(v), g, None, None) == _lib.ABO_EINVAL
    assert L.abo_nlml_grad_ard(m._require(), 0, C.byref(v), g, None, None) == _lib.ABO_EINVAL
    X33 = synth.points(2, 20, 33)
    m33 = abo.update(abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 2.0), 1e-2), X33, synth.objective(X33))
    assert L.abo_nlml_grad_ard(m33._require(), 33, C.byref(v), g, None, None) == _lib.ABO_EINVAL
    assert L.abo_nlml_grad_ard(None, 3, C.byref(v), g, None, None) == _lib.ABO_EINVAL
    # not fitted
    hp, prm = C.c_void_p(), gp._params()
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    try:
        assert L.abo_nlml_grad_ard(hp, 3, C.byref(v), g, None, None) == _lib.ABO_EINVAL
    finally:
        L.abo_destroy(hp)
    # an appended view
    m2 = abo.append(m, np.array([0.1, 0.2, 0.3]), 0.5)
    assert L.abo_nlml_grad_ard(m2._require(), 3, C.byref(v), g, None, None) == _lib.ABO_EINVAL
    # a gradient-enhanced handle
    Xg = synth.points(1, 12, 2)
    Yg = np.column_stack([np.sin(Xg).sum(1), np.cos(Xg)])
    mg = abo.update(abo.GradientGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.7), 3, 1e-3), Xg, Yg)
    assert L.abo_nlml_grad_ard(mg._require(), 2, C.byref(v), g, None, None) == _lib.ABO_EINVAL


ELLS4 = np.array([0.3, 1.7, 0.08, 6.0])


@pytest.fixture(scope="module")
def round_trip():
    N, d = 60, 4
    X, y = synth.standardized_problem(N, d, 0.02)
    X = X * np.array([1.0, 4.0, 0.2, 10.0])                       # a box that is not the unit cube
    kern = lambda ell: 1.3 * abo.with_lengthscale(abo.Matern52Kernel(), ell)
    ard = abo.update(abo.HipStandardGP(kern(ELLS4), 1e-3), X, y)
    hand = abo.update(abo.HipStandardGP(kern(1.0), 1e-3), X / ELLS4, y)          # isotropic, fitted on hand-scaled data
    Z = synth.points(7, 3000, d) * np.array([1.0, 4.0, 0.2, 10.0])
    return X, y, ard, hand, Z


def test_python_round_trip_posterior_and_training_data(round_trip):
    import torch
    X, y, ard, hand, Z = round_trip
    st = A.fit(O.MATERN52, ELLS4, 1.3, 1e-3, 0.0, X, y)
    mu, var = O.predict(st, Z / ELLS4)
    for z in (Z, torch.from_numpy(Z).cuda()):
        m, v = abo.mean_and_var(ard, z)
        m, v = (m.cpu().numpy(), v.cpu().numpy()) if hasattr(m, "cpu") else (m, v)
        assert np.max(np.abs(m - mu)) < 1e-9 and np.max(np.abs(v - var)) < 1e-9
        np.testing.assert_array_equal(m, abo.posterior_mean(hand, Z / ELLS4))
    np.testing.assert_array_equal(abo.posterior_var(ard, Z), abo.posterior_var(hand, Z / ELLS4))
    um, uv = abo.unstandardized_mean_and_var(ard, Z, (2.0, 3.0))
    np.testing.assert_allclose(um, mu * 3.0 + 2.0, atol=1e-8)
    assert abs(abo.nlml_fitted(ard) - O.nlml(st)) <= 1e-9 * max(1.0, abs(O.nlml(st)))
    # (exp(log ℓ) is ℓ to an ulp only)
    assert abs(abo.nlml(ard, list(np.log(ELLS4)) + [math.log(1.3)], X, y) - abo.nlml_fitted(ard)) <= 1e-12 * abs(abo.nlml_fitted(ard))
    Xb, yb = abo.training_data(ard)
    np.testing.assert_allclose(Xb, X, rtol=4e-16, atol=0)
    np.testing.assert_array_equal(yb, y)
    # update through the bordered appends: the new rows are scaled like the old ones
    inc = abo.HipStandardGP(1.3 * abo.with_lengthscale(abo.Matern52Kernel(), ELLS4), 1e-3, n_max=128, incremental_update=True)
    m0 = abo.update(inc, X[:57], y[:57])                       # three new rows: within the append rule at this size
    m1 = abo.update(m0, X, y)
    assert m1.update_path == "appended"
    np.testing.assert_allclose(abo.posterior_mean(m1, Z[:200]), mu[:200], atol=1e-8)


def test_python_round_trip_evaluate_matches_hand_scaled_model(round_trip):
    import torch
    X, y, ard, hand, Z = round_trip
    ystar = np.array([y.min() - 0.3, y.min() - 0.1, y.min() - 0.6])
    acqs = [abo.ExpectedImprovement(0.01, float(y.min())), abo.LogExpectedImprovement(0.01, float(y.min())), abo.UpperConfidenceBound(2.0),
            abo.ProbabilityImprovement(0.01, float(y.min())), abo.MaxValueEntropySearch(ystar),
            abo.EnsembleAcquisition([0.3, 0.7], [abo.ExpectedImprovement(0.01, float(y.min())), abo.UpperConfidenceBound(1.5)])]
    for acq in acqs:
        s1, v1, i1 = abo.evaluate(acq, ard, Z, k=25)
        s2, v2, i2 = abo.evaluate(acq, hand, Z / ELLS4, k=25)
        np.testing.assert_array_equal(i1, i2)
        np.testing.assert_array_equal(v1, v2)
        np.testing.assert_array_equal(s1, s2)
        np.testing.assert_array_equal(acq(ard, Z), s2)
    zt = torch.from_numpy(Z).cuda()
    _, v3, i3 = abo.evaluate(acqs[0], ard, zt, k=25, return_scores=False)
    _, v2, i2 = abo.evaluate(acqs[0], hand, Z / ELLS4, k=25)
    np.testing.assert_array_equal(i3.cpu().numpy(), i2)
    m2, s2, v4, i4 = abo.update_and_evaluate(acqs[0], ard, X, y, Z, k=25)
    np.testing.assert_array_equal(i4, i2)
    np.testing.assert_allclose(v4, v2, rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(abo.posterior_mean(m2, Z), abo.posterior_mean(ard, Z))


def test_python_round_trip_optimize_acquisition_device(round_trip):
    X, y, ard, hand, Z = round_trip
    lower, upper = np.zeros(4), np.array([1.0, 4.0, 0.2, 10.0])
    dom = abo.ContinuousDomain(lower, upper)
    ystar = np.array([y.min() - 0.3, y.min() - 0.1])
    for acq in (abo.ExpectedImprovement(0.01, float(y.min())), abo.MaxValueEntropySearch(ystar)):
        best, val, sx, sv, rx, rv = abo.optimize_acquisition_device(acq, ard, dom, n_grid=2000, n_local=16, seed=3, return_all=True)
        assert np.all(best >= lower) and np.all(best <= upper)
        assert np.all(sx >= lower) and np.all(sx <= upper) and np.all(rx >= lower) and np.all(rx <= upper)
        # the value test_gpu_refine.py's bar: rtol 1e-8, atol 1e-9
        np.testing.assert_allclose(acq(ard, best[None, :])[0], val, rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(acq(ard, sx), sv, rtol=1e-8, atol=1e-9)
        # the same call on the hand-scaled model in the scaled box: the same points, multiplied back
        hb, hval, *_ = abo.optimize_acquisition_device(acq, hand, abo.ContinuousDomain(lower / ELLS4, upper / ELLS4), n_grid=2000,
                                                       n_local=16, seed=3, return_all=True)
        assert hval == val
        np.testing.assert_allclose(best, hb * ELLS4, rtol=4e-16, atol=0)
    # the refinement alone, from starts in the caller's coordinates: inside the box, no start ends below its grid score, and the
    # returned values are the acquisition's at the returned points
    xr, fr = abo.refine_starts(acq, ard, sx, lower, upper)
    assert np.all(xr >= lower) and np.all(xr <= upper) and np.all(fr >= sv - 1e-9)
    np.testing.assert_allclose(acq(ard, xr), fr, rtol=1e-8, atol=1e-9)


def test_ard_hyperparameter_search_end_to_end():
    """N = 80, d = 4, Matérn-5/2, an objective of the first two coordinates only (ard_oracle.two_coordinate_problem, seed 11 — the seed
    tests/test_ard_cpu.py checks with SciPy on the checker's NLML alone, with and without the box).  Started from the isotropic
    optimum, the ARD search must not end above it, and both irrelevant length scales must end above both relevant ones."""
    X, y = A.two_coordinate_problem(11)
    dom = abo.ContinuousDomain(np.zeros(4), np.ones(4))
    m = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.5), 1e-4)
    iso = abo.optimize_hyperparameters(m, X, y, [math.log(0.5), 0.0], domain=dom, rng=np.random.default_rng(0))
    p_iso = [math.log(abo.get_lengthscale(iso)[0]), math.log(abo.get_scale(iso)[0])]
    v_iso = abo.nlml(iso, p_iso, X, y)
    ard = abo.optimize_hyperparameters(iso, X, y, p_iso, domain=dom, rng=np.random.default_rng(0), ard=True)
    assert ard is not iso and ard.gpx is None and abo.ard_lengthscales(ard) is not None
    ell = np.array(abo.get_lengthscale(ard))
    v_ard = abo.nlml(ard, list(np.log(ell)) + [math.log(abo.get_scale(ard)[0])], X, y)
    print("isotropic", abo.get_lengthscale(iso), v_iso, "ARD", ell, v_ard)
    assert v_ard <= v_iso
    assert ell[2:].min() > ell[:2].max()
    # the device's value and gradient at the result are the checker's
    p = np.append(np.log(ell), math.log(abo.get_scale(ard)[0]))
    v, g = abo.nlml_and_grad_ard(ard, p, X, y)
    rv, rg = A.stub_nlml_and_grad_ard(ard, p, X, y)
    assert abs(v - rv) <= 1e-9 * max(1.0, abs(rv))
    np.testing.assert_allclose(g, rg, rtol=0, atol=1e-6 * max(1.0, abs(rv)))
