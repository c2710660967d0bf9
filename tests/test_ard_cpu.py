"""ARD length scales (one per coordinate), host side — no device work.

The checker is tests/ard_oracle.py: the ARD kernel is the isotropic one with ℓ = 1 on coordinates divided by ℓ_c, its analytic
gradient is computed densely.  Here: the checker against its own central differences, the kernel / model plumbing of the vector
length scale, the two scaling helpers, the refusals of the entry points that do not scale, and the ARD hyper-parameter search with the
device call answered by the checker."""
import math

import numpy as np
import pytest
import torch

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import hyperparams as H
from abstractbayesopt.jl_amd import incremental, kernels, thompson
from oracle import gp_oracle as O
from tests import ard_oracle as A

FAMILIES = [O.SE, O.MATERN52, O.MATERN72, O.MATERN32]
ELLS4 = (0.3, 1.7, 0.08, 6.0)          # spread over two decades


@pytest.mark.parametrize("family", FAMILIES)
def test_helper_gradient_against_its_own_central_differences(family):
    """h = 1e-5, rtol 2e-6, atol 1e-6·max(1, |v|): the bars of test_nlml_gradient_against_oracle_finite_differences"""
    rng = np.random.default_rng(5)
    X = rng.random((40, 4))
    y = np.sin(3.0 * X[:, 0]) + X[:, 2] + 0.05 * rng.standard_normal(40)
    sf2, noise, mean_c = 1.7, 1e-2, 0.3
    v, g_ell, g_sf2, g_noise = A.nlml_and_grad(family, ELLS4, sf2, noise, mean_c, X, y)
    fd_ell, fd_sf2, fd_noise = A.central_differences(family, ELLS4, sf2, noise, mean_c, X, y, h=1e-5)
    atol = 1e-6 * max(1.0, abs(v))
    np.testing.assert_allclose(g_ell, fd_ell, rtol=2e-6, atol=atol)
    np.testing.assert_allclose([g_sf2, g_noise], [fd_sf2, fd_noise], rtol=2e-6, atol=atol)
    # at equal length scales the partials add up to the isotropic derivative (central difference of the isotropic NLML)
    _, g_iso, _, _ = A.nlml_and_grad(family, [0.6] * 4, sf2, noise, mean_c, X, y)
    f = lambda le: O.nlml(O.fit(family, math.exp(le), sf2, noise, mean_c, X, y))
    fd = (f(math.log(0.6) + 1e-5) - f(math.log(0.6) - 1e-5)) / 2e-5
    np.testing.assert_allclose(g_iso.sum(), fd, rtol=2e-6, atol=atol)


def test_vector_lengthscale_round_trips_and_crosses_the_abi_as_one():
    k = 2.5 * abo.with_lengthscale(abo.Matern52Kernel(), np.array(ELLS4))
    inner, scale, ell = kernels.extract_scale_and_lengthscale(k)
    assert inner == abo.Matern52Kernel() and scale == 2.5 and ell == ELLS4 and isinstance(ell, tuple)
    assert "(0.3, 1.7, 0.08, 6.0)" in repr(k)
    gp = abo.HipStandardGP(k, 0.1)
    assert gp._params().ell == 1.0 and gp._params().sigma_f2 == 2.5
    assert abo.get_lengthscale(gp) == list(ELLS4) and abo.get_scale(gp) == [2.5]
    np.testing.assert_array_equal(abo.ard_lengthscales(gp), ELLS4)
    r = abo.rescale_model(gp, 2.0)
    assert abo.get_lengthscale(r) == list(ELLS4) and abo.get_scale(r) == [0.625]
    for bad in ([], [1.0, 0.0], [1.0, -2.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            abo.with_lengthscale(abo.Matern52Kernel(), bad)


def test_scalar_kernel_is_unchanged():
    k = 4.0 * abo.with_lengthscale(abo.Matern52Kernel(), 2.0)
    assert k.lengthscale == 2.0 and isinstance(k.lengthscale, float) and "ℓ = 2.0" in repr(k)
    gp = abo.HipStandardGP(k, 0.1)
    p = gp._params()
    assert (p.ell, p.sigma_f2, p.noise_var, p.family) == (2.0, 4.0, 0.1, kernels.MATERN52)
    assert abo.ard_lengthscales(gp) is None and abo.get_lengthscale(gp) == [2.0]
    x = np.arange(6.0).reshape(3, 2)
    assert abo.to_model_space(gp, x) is x and abo.from_model_space(gp, x) is x       # untouched, not copied
    t = torch.arange(6.0, dtype=torch.float64).reshape(3, 2)
    assert abo.to_model_space(gp, t) is t


def test_scaling_helpers_numpy_and_torch():
    gp = abo.HipStandardGP(abo.with_lengthscale(abo.SqExponentialKernel(), ELLS4), 0.1)
    e = np.array(ELLS4)
    X = np.random.default_rng(0).random((7, 4))
    Xs = abo.to_model_space(gp, X)
    assert isinstance(Xs, np.ndarray)
    np.testing.assert_array_equal(Xs, X / e)
    np.testing.assert_allclose(abo.from_model_space(gp, Xs), X, rtol=4e-16, atol=0)
    np.testing.assert_array_equal(abo.to_model_space(gp, [list(r) for r in X]), X / e)      # a vector of d-vectors
    t = torch.from_numpy(X)
    ts = abo.to_model_space(gp, t)
    assert isinstance(ts, torch.Tensor) and ts.device == t.device and ts.dtype == torch.float64
    np.testing.assert_array_equal(ts.numpy(), X / e)
    np.testing.assert_array_equal(abo.from_model_space(gp, ts).numpy(), (X / e) * e)
    # a box bound is ONE d-vector, not d points of dimension 1
    np.testing.assert_array_equal(abo.to_model_space(gp, np.ones(4), bounds=True), 1.0 / e)
    np.testing.assert_array_equal(abo.from_model_space(gp, np.ones(4), bounds=True), e)
    # d = 1: the reference's vector of reals
    g1 = abo.HipStandardGP(abo.with_lengthscale(abo.SqExponentialKernel(), [0.25]), 0.1)
    np.testing.assert_array_equal(abo.to_model_space(g1, [1.0, 2.0, 3.0]), [4.0, 8.0, 12.0])
    np.testing.assert_array_equal(abo.to_model_space(g1, np.array([[1.0], [2.0]])), [[4.0], [8.0]])
    np.testing.assert_array_equal(abo.to_model_space(g1, 0.5), [2.0])


def test_wrong_length_vector_is_rejected():
    gp = abo.HipStandardGP(abo.with_lengthscale(abo.SqExponentialKernel(), ELLS4), 0.1)
    for bad in (np.zeros((5, 3)), np.zeros(5), torch.zeros((5, 6), dtype=torch.float64), [[0.0, 1.0], [1.0, 2.0]]):
        with pytest.raises(abo.DimensionMismatch):
            abo.to_model_space(gp, bad)
    with pytest.raises(abo.DimensionMismatch):
        abo.to_model_space(gp, np.zeros(3), bounds=True)
    # the entry points check before any device work
    with pytest.raises(abo.DimensionMismatch):
        abo.update(gp, np.zeros((5, 3)), np.zeros(5))
    with pytest.raises(abo.DimensionMismatch):
        abo.posterior_mean(gp, np.zeros((5, 3)))
    with pytest.raises(abo.DimensionMismatch):
        abo.evaluate(abo.UpperConfidenceBound(2.0), gp, np.zeros((5, 3)))
    with pytest.raises(abo.DimensionMismatch):
        abo.optimize_acquisition_device(abo.UpperConfidenceBound(2.0), gp, abo.ContinuousDomain([0.0] * 3, [1.0] * 3))


def test_entry_points_that_do_not_scale_refuse_an_ard_model():
    k = abo.with_lengthscale(abo.Matern52Kernel(), ELLS4)
    gp = abo.HipStandardGP(k, 0.1)
    Z = np.zeros((8, 4))
    calls = {
        "append": lambda: incremental.append(gp, np.zeros(4), 0.0),
        "ResidentCandidates": lambda: incremental.ResidentCandidates(gp, Z),
        "greedy_qei": lambda: incremental.greedy_qei(gp, None, 2, 0.01, 0.0),
        "mc_qei": lambda: incremental.mc_qei(gp, None, 2, 0.01, 0.0),
        "sample_paths": lambda: thompson.sample_paths(gp, 4),
        "max_value_samples": lambda: thompson.max_value_samples(gp, Z, 4),
        "thompson_batch": lambda: thompson.thompson_batch(gp, Z, 2),
        "SamplePaths": lambda: thompson.SamplePaths(gp, None, None, None, None),
        "HipShardedGP": lambda: abo.HipShardedGP(k, 0.1, devices=(0,)),
        "HipShardedGradientGP": lambda: abo.HipShardedGradientGP(k, 5, 0.1, devices=(0,)),
        "HipGradientGP": lambda: abo.HipGradientGP(k, 5, 0.1),
    }
    for what, call in calls.items():
        with pytest.raises(abo.ArdUnsupported, match="does not support ARD length scales"):
            call()
    assert issubclass(abo.ArdUnsupported, TypeError)
    with pytest.raises(TypeError):
        abo.optimize_hyperparameters(abo.HipGradientGP(abo.Matern52Kernel(), 5, 0.1), Z, np.zeros((8, 5)), [0.0] * 5, ard=True)


def test_ard_hyperparameter_search_with_the_device_call_stubbed(monkeypatch):
    """seed 11 of ard_oracle.two_coordinate_problem (the one tests/test_gpu_ard.py runs on the device): SciPy on the helper's NLML
    alone ends below the isotropic optimum and with both irrelevant length scales above both relevant ones"""
    monkeypatch.setattr(H, "nlml_and_grad_ard", A.stub_nlml_and_grad_ard)
    monkeypatch.setattr(H, "nlml_and_grad", A.stub_nlml_and_grad)
    X, y = A.two_coordinate_problem(11)
    m = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.5), 1e-4)
    iso = abo.optimize_hyperparameters(m, X, y, [math.log(0.5), 0.0], rng=np.random.default_rng(0))
    p_iso = [math.log(abo.get_lengthscale(iso)[0]), math.log(abo.get_scale(iso)[0])]
    v_iso = A.stub_nlml_and_grad(iso, p_iso, X, y)[0]
    ard = abo.optimize_hyperparameters(iso, X, y, p_iso, rng=np.random.default_rng(0), ard=True)
    assert ard is not iso and ard.gpx is None and abo.ard_lengthscales(ard) is not None
    ell = np.array(abo.get_lengthscale(ard))
    assert ell.shape == (4,)
    v_ard = A.stub_nlml_and_grad_ard(ard, list(np.log(ell)) + [math.log(abo.get_scale(ard)[0])], X, y)[0]
    assert v_ard <= v_iso                         # L-BFGS-B does not go uphill from its start
    assert ell[2:].min() > ell[:2].max()
    # the start may be given as the d + 1 vector too, and length_scale_only keeps the scale
    again = abo.optimize_hyperparameters(iso, X, y, [p_iso[0]] * 4 + [p_iso[1]], rng=np.random.default_rng(0), ard=True)
    np.testing.assert_allclose(abo.get_lengthscale(again), ell, rtol=1e-12)
    ls = abo.optimize_hyperparameters(iso, X, y, p_iso, rng=np.random.default_rng(0), ard=True, length_scale_only=True)
    assert abo.get_scale(ls) == abo.get_scale(iso) and len(abo.get_lengthscale(ls)) == 4
    with pytest.raises(abo.DimensionMismatch):
        abo.optimize_hyperparameters(iso, X, y, [0.0, 0.0, 0.0], ard=True)
