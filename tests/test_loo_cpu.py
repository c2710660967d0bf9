"""Leave-one-out cross-validation, host side — no device work.

The checker is tests/loo_oracle.py.  Here: its closed form against its own brute force (N refits), its dense gradient against central
differences of its value, the three places that name the two new entry points (header, ctypes binding, Julia shim), the refusal of
objective="loo" with ard=True, and the objective="loo" search with the device call answered by the checker."""
import math
import os
import re

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import hyperparams as H
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O
from tests import loo_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "integration", "julia", "LeaveOneOut.jl")
FAMILIES = [O.SE, O.MATERN52, O.MATERN72, O.MATERN32]
SF2, NOISE, MEAN_C, ELL = 1.7, 1e-2, 0.3, 0.6


def problem(N, d, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    return X, np.sin(3.0 * X[:, 0]) + X[:, -1] + 0.05 * rng.standard_normal(N) + 0.3


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N", [1, 2, 17, 60])
def test_closed_form_agrees_with_brute_force(family, N):
    """fp64 on both sides and a condition number of at most a few 1e4: 1e-11, scaled as the device tests scale"""
    X, y = problem(N, 3)
    mu, var, lpd, v = LO.closed_form(family, ELL, SF2, NOISE, MEAN_C, X, y)
    bmu, bvar, blpd, bv = LO.brute_force(family, ELL, SF2, NOISE, MEAN_C, X, y)
    assert np.max(np.abs(mu - bmu) / np.maximum(1.0, np.abs(bmu))) <= 1e-11
    assert np.max(np.abs(var - bvar)) / SF2 <= 1e-11
    assert np.max(np.abs(lpd - blpd) / np.maximum(1.0, np.abs(blpd))) <= 1e-9
    assert abs(v - bv) <= 1e-10 * max(1.0, abs(bv))
    if N == 1:
        assert bmu[0] == MEAN_C and bvar[0] == SF2 + NOISE


@pytest.mark.parametrize("family", FAMILIES)
def test_gradient_agrees_with_central_differences(family):
    """h = 1e-5, rtol 2e-6, atol 1e-6·max(1, |v|): the bars of test_nlml_gradient_against_oracle_finite_differences"""
    X, y = problem(40, 4)
    v, g_ell, g_sf2, g_noise = LO.nlpl_and_grad(family, ELL, SF2, NOISE, MEAN_C, X, y)
    fd = LO.central_differences(family, ELL, SF2, NOISE, MEAN_C, X, y, h=1e-5)
    np.testing.assert_allclose([g_ell, g_sf2, g_noise], fd, rtol=2e-6, atol=1e-6 * max(1.0, abs(v)))
    # without noise the noise partial vanishes and there is nothing to difference
    v0, _, _, g0 = LO.nlpl_and_grad(family, 0.2, SF2, 0.0, MEAN_C, X[:17], y[:17])
    assert g0 == 0.0 and LO.central_differences(family, 0.2, SF2, 0.0, MEAN_C, X[:17], y[:17])[2] is None


def test_header_binding_and_shim_name_the_same_two_functions():
    from tests import test_julia_shim_cpu as J
    protos = J.c_prototypes()
    names = ("abo_loo", "abo_loo_grad")
    lib = abo._lib.lib()
    for name in names:
        assert name in protos and name in abo._lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == len(protos[name])
    assert [len(protos[n]) for n in names] == [6, 5]
    calls = [c for c in J.julia_calls(JL) if c[0] in names]
    assert {c[0] for c in calls} == set(names)
    for name, types, ret, line in J.julia_calls(JL):
        assert ret == "Int32" and len(types) == len(protos[name]), (name, line)
        assert all(J.jl_matches_c(t, c) for t, c in zip(types, protos[name])), (name, line)
    assert 'include("LeaveOneOut.jl")' in open(J.SHIMS[0]).read()
    assert re.search(r"^function leave_one_out\(m::HipStandardGP\)", open(JL).read(), flags=re.M)
    for name in ("leave_one_out", "loo_and_grad"):
        assert callable(getattr(abo, name))


def test_loo_objective_with_ard_raises():
    m = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.5), 1e-2)
    X, y = problem(20, 3)
    with pytest.raises(ValueError, match="ARD"):
        abo.optimize_hyperparameters(m, X, y, [0.0, 0.0], ard=True, objective="loo")
    with pytest.raises(ValueError, match="objective"):
        abo.optimize_hyperparameters(m, X, y, [0.0, 0.0], objective="cv")
    with pytest.raises(TypeError):
        abo.optimize_hyperparameters(abo.HipGradientGP(abo.Matern52Kernel(), 4, 0.1), X, np.zeros((20, 4)), [0.0, 0.0], objective="loo")


def stub_loo_and_grad(model, params, xs, ys):
    """`hyperparams.loo_and_grad` answered by the checker instead of the device (same signature and parameter order)"""
    v, g_ell, g_sf2, _ = LO.nlpl_and_grad(model.kernel.family, math.exp(params[0]), math.exp(params[1]), model.noise_var,
                                          float(getattr(model.mean, "c", 0.0)), xs, ys)
    return v, np.array([g_ell, g_sf2])


def test_loo_search_with_the_device_call_stubbed(monkeypatch):
    """objective="loo" reaches loo_and_grad (and only it), keeps bounds and failure handling, and does not go uphill from its start"""
    monkeypatch.setattr(H, "loo_and_grad", stub_loo_and_grad)
    monkeypatch.setattr(H, "nlml_and_grad", lambda *a: (_ for _ in ()).throw(AssertionError("the NLML objective was evaluated")))
    X, y = synth.standardized_problem(64, 3, 0.3)              # (the problem tests/test_gpu_loo.py searches on the device)
    m = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 2.0), 0.09)
    start = [math.log(2.0), 0.0]
    out = abo.optimize_hyperparameters(m, X, y, start, objective="loo", rng=np.random.default_rng(0))
    assert out is not m and out.gpx is None
    p = [math.log(abo.get_lengthscale(out)[0]), math.log(abo.get_scale(out)[0])]
    assert stub_loo_and_grad(out, p, X, y)[0] < stub_loo_and_grad(m, start, X, y)[0]
    ls = abo.optimize_hyperparameters(m, X, y, start, objective="loo", length_scale_only=True, rng=np.random.default_rng(0))
    assert abo.get_scale(ls) == abo.get_scale(m)
