"""CPU tests of Thompson sampling's host half (abstractbayesopt.jl_amd/thompson.py) and of the abo_paths_* surface
(include/abo_hip.h): declaration, export and binding of the new names, argument validation without a device, the frequency law of
the four kernel families, seeded base draws, the de-duplication of a batch, and the definition's statistics restated on the CPU
oracle (a pathwise sample has the posterior's mean and variance)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import thompson
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["abo_paths_create", "abo_paths_destroy", "abo_paths_eval", "abo_paths_eval_cand", "abo_paths_stats_get"]
KERNELS = {O.SE: abo.SqExponentialKernel, 1: abo.Matern52Kernel, 2: abo.ApproxMatern72Kernel, 3: abo.Matern32Kernel}


def test_new_names_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abo_hip.h")).read()
    lib = abo._lib.lib()
    for name in NAMES:
        assert re.search(r"^int32_t\s+%s\s*\(" % name, hdr, flags=re.M), f"{name} is not declared in the header"
        assert name in abo._lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, f"{name} has no argtypes"
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr)                       # new entry points only
    assert C.sizeof(abo._lib.AboPathsStats) == 6 * 8
    for name in ("SamplePaths", "sample_paths", "spectral_frequencies", "thompson_batch"):
        assert hasattr(abo, name)


def test_argument_validation_needs_no_device():
    lib, EINVAL = abo._lib.lib(), abo._lib.ABO_EINVAL
    buf = np.zeros(64)
    p, hp = buf.ctypes.data, C.c_void_p()
    fake = C.c_void_p(buf.ctypes.data)                  # a non-null "handle": every range check comes before it is looked at
    assert lib.abo_paths_create(None, 4, 8, p, p, p, p, 0, C.byref(hp)) == EINVAL and "null" in abo._lib.last_error()
    assert lib.abo_paths_create(fake, 4, 8, None, p, p, p, 0, C.byref(hp)) == EINVAL and "null" in abo._lib.last_error()
    assert lib.abo_paths_create(fake, 4, 8, p, p, p, p, 0, None) == EINVAL and "null" in abo._lib.last_error()
    for S in (0, -1, 257):
        assert lib.abo_paths_create(fake, S, 8, p, p, p, p, 0, C.byref(hp)) == EINVAL and "1..256" in abo._lib.last_error()
    for R in (0, 65537):
        assert lib.abo_paths_create(fake, 4, R, p, p, p, p, 0, C.byref(hp)) == EINVAL and "1..65536" in abo._lib.last_error()
    assert lib.abo_paths_create(fake, 4, 8, p, p, p, p, 7, C.byref(hp)) == EINVAL and "memory space" in abo._lib.last_error()
    assert hp.value is None
    assert lib.abo_paths_eval(None, p, 1, 1, 0, 0, p, 0, None, None, 0) == EINVAL and "null" in abo._lib.last_error()
    assert lib.abo_paths_eval_cand(None, fake, 0, p, 0, None, None, 0) == EINVAL and "null" in abo._lib.last_error()
    assert lib.abo_paths_stats_get(None, None) == EINVAL
    assert lib.abo_paths_destroy(None) == abo._lib.ABO_OK


def test_python_layer_refuses_what_it_cannot_serve():
    class Sharded:
        devices = [0, 1]
    with pytest.raises(TypeError, match="sharded"):
        abo.sample_paths(Sharded(), 4)
    with pytest.raises(TypeError):
        abo.sample_paths(object(), 4)
    with pytest.raises(ValueError):                     # gpx === nothing
        abo.sample_paths(abo.HipStandardGP(abo.SqExponentialKernel(), 0.1), 4)
    with pytest.raises(ValueError):
        abo.spectral_frequencies(abo.SqExponentialKernel(), 0, 2)


@pytest.mark.parametrize("family", [0, 1, 2, 3])
def test_spectral_frequencies_reproduce_the_kernel(family):
    """φ(x)ᵀφ(z) → k(x, z): R = 16 384, 40 × 40 random pairs in [0,1]⁴, ℓ = 0.7; max error / σ_f² ≤ 8 / sqrt(R) (the per-entry standard
    deviation of the estimate is below 1 / sqrt(R): 2·cos·cos has variance ≤ 1)."""
    R, d, ell, sf2 = 16384, 4, 0.7, 1.7
    rng = np.random.default_rng(100 + family)
    omega = abo.spectral_frequencies(KERNELS[family](), R, d, rng)
    assert omega.shape == (R, d)
    phase = rng.uniform(0.0, 2.0 * np.pi, R)
    X, Z = rng.random((40, d)), rng.random((40, d))
    fx = math.sqrt(2.0 * sf2 / R) * np.cos(X @ omega.T / ell + phase)
    fz = math.sqrt(2.0 * sf2 / R) * np.cos(Z @ omega.T / ell + phase)
    err = np.max(np.abs(fx @ fz.T - O.kernel_matrix(family, ell, sf2, X, Z))) / sf2
    print(f"family {family}: max error {err * math.sqrt(R):.2f} / sqrt(R)")
    assert err <= 8.0 / math.sqrt(R)


def test_seeded_base_draws_are_reproducible_and_shaped():
    k = abo.Matern52Kernel()
    a = thompson.draw_base(k, 5, 64, 33, 3, 7)
    b = thompson.draw_base(k, 5, 64, 33, 3, np.random.default_rng(7))
    c = thompson.draw_base(k, 5, 64, 33, 3, 8)
    assert [x.shape for x in a] == [(64, 3), (64,), (5, 64), (5, 33)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], c[0])
    assert np.all((a[1] >= 0.0) & (a[1] < 2.0 * np.pi))


def test_batch_deduplication_on_a_stubbed_result():
    top = np.array([[5, 2, 9], [5, 7, 1], [5, 7, 3], [4, 5, 7]])
    assert thompson.distinct_picks(top).tolist() == [5, 7, 3, 4]
    assert thompson.distinct_picks(np.array([[3, -1], [3, 8]])).tolist() == [3, 8]
    with pytest.raises(ValueError, match="no candidate left"):
        thompson.distinct_picks(np.array([[1, -1], [1, -1]]))


def test_pathwise_samples_have_the_posterior_moments_on_the_oracle():
    """The definition means what it claims: N = 30, d = 4, noise 1e-2, R = 4096, 20 000 paths in batches of 256 — path mean and variance
    at 6 test points agree with the oracle's posterior within 5 standard errors of the mean and 15 % of the variance.  The four formulas of
    the header, restated in NumPy on oracle.gp_oracle.fit / kernel_matrix."""
    fam, ell, sf2, noise, c, N, d, R = 1, 0.6, 1.3, 1e-2, 0.4, 30, 4, 4096
    rng = np.random.default_rng(5)
    X, Z = rng.random((N, d)), rng.random((6, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(N)
    st = O.fit(fam, ell, sf2, noise, c, X, y)
    mu, var = O.predict(st, Z)
    Kzx = O.kernel_matrix(fam, ell, sf2, Z, X)
    import scipy.linalg as sla
    tot, tot2, n = np.zeros(6), np.zeros(6), 0
    for _ in range(79):                                 # 79 × 256 = 20 224 paths
        omega, phase, w, eps = thompson.draw_base(KERNELS[fam](), 256, R, N, d, rng)
        sc = math.sqrt(2.0 * sf2 / R)
        fX = c + w @ (sc * np.cos(X @ omega.T / ell + phase)).T
        fZ = c + w @ (sc * np.cos(Z @ omega.T / ell + phase)).T
        V = sla.cho_solve((st.L, True), (y[None, :] - fX - math.sqrt(noise) * eps).T)
        g = fZ + (Kzx @ V).T
        tot += g.sum(axis=0); tot2 += (g * g).sum(axis=0); n += g.shape[0]
    m = tot / n
    v = tot2 / n - m * m
    se = np.abs(m - mu) / np.sqrt(var / n)
    print("standard errors", np.round(se, 2), "variance ratio", np.round(v / var, 3))
    assert np.all(se <= 5.0)
    assert np.all(np.abs(v / var - 1.0) <= 0.15)


def test_julia_wrappers_bind_the_entry_points_and_match_the_header():
    """integration/julia/HipStandardGP.jl binds create / eval / eval_cand / destroy; every such call agrees with the header under the
    shim test's own parser (tests/test_julia_shim_cpu.py checks the whole file the same way)"""
    from tests import test_julia_shim_cpu as J
    protos = J.c_prototypes()
    calls = [c for c in J.julia_calls(J.SHIMS[0]) if c[0].startswith("abo_paths_")]
    assert {c[0] for c in calls} == {"abo_paths_create", "abo_paths_destroy", "abo_paths_eval", "abo_paths_eval_cand"}
    for name, types, ret, line in calls:
        assert ret == "Int32" and len(types) == len(protos[name]), (name, line)
        assert all(J.jl_matches_c(t, c) for t, c in zip(types, protos[name])), (name, line)
    code = open(J.SHIMS[0]).read()
    for fn in ("function sample_paths(", "function thompson_batch(", "function path_argmin(", "function spectral_frequencies("):
        assert fn in code


def test_sample_paths_checks_the_base_arrays_against_the_model(monkeypatch):
    monkeypatch.setattr(thompson, "_model_shape", lambda model: (10, 3))
    m = abo.HipStandardGP(abo.SqExponentialKernel(), 0.1)
    om, ph, w, eps = thompson.draw_base(abo.SqExponentialKernel(), 4, 8, 10, 3, 0)
    for bad in ((om[:, :2], ph, w, eps), (om, ph[:7], w, eps), (om, ph, w, eps[:, :9]), (om, ph, w[0], eps)):
        with pytest.raises(ValueError, match="SamplePaths"):
            abo.SamplePaths(m, *bad)
