"""CPU tests of abo_remove / remove_points (no GPU needed): the identities of DESIGN.md "Removing an observation", restated in NumPy
in the kernels' scan order (tests/remove_oracle.py), against numpy.linalg refits for every j of a small N; the chunked scan against
the sequential one; the argument handling of remove_points; the C-ABI declared, exported, bound by _lib.py and the Julia shim with
the header's prototype, and refusing bad arguments before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import incremental
from tests import remove_oracle as R
from tests.test_julia_shim_cpu import c_prototypes, jl_matches_c, julia_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def _problem(N, d=3, noise=1e-3, sf2=1.3, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    D = ((X[:, None] - X[None]) ** 2).sum(-1)
    return sf2 * np.exp(-0.5 * D / 0.6 ** 2) + noise * np.eye(N), rng.standard_normal(N)


@pytest.fixture(scope="module")
def small():
    Kt, delta = _problem(70)
    return Kt, delta, R.refit(Kt, delta)


def _bars(Kt):
    """what rounding allows: ε·cond(K̃) on everything that goes through K̃⁻¹ (both the update and the numpy refit carry it), a few
    hundred ε on L itself (each entry of L′ is one fused product and a sum of ≤ N products of entries of L)"""
    cond = np.linalg.cond(Kt)
    return 64 * EPS * np.sqrt(cond) * np.max(np.abs(Kt)) ** 0.5, 64 * EPS * cond


@pytest.mark.parametrize("chunk", [R.CHUNK, None])
def test_identities_match_refits_for_every_j(small, chunk):
    Kt, delta, (L, W, alpha, logdet, quad) = small
    N = Kt.shape[0]
    bar_L, bar_inv = _bars(Kt)
    for j in range(N):
        keep = np.r_[0:j, j + 1:N]
        Lr, Wr, ar, ldr, qr = R.refit(Kt[np.ix_(keep, keep)], delta[keep])
        Ln, Wn, an, ldn, qn = R.remove(L, W, alpha, logdet, quad, j, chunk)
        assert np.max(np.abs(Ln - Lr)) <= bar_L, j
        assert np.max(np.abs(np.triu(Ln, 1))) == 0.0 and np.max(np.abs(np.triu(Wn, 1))) == 0.0
        assert np.max(np.abs(Wn @ Lr - np.eye(N - 1))) <= bar_inv, j
        assert np.max(np.abs(an - ar)) / np.max(np.abs(ar)) <= bar_inv, j
        assert abs(ldn - ldr) <= bar_inv * N and abs(qn - qr) / abs(qr) <= bar_inv, j
        # rows and columns in front of j are copies, bit for bit
        np.testing.assert_array_equal(Ln[:j, :j], L[:j, :j])
        np.testing.assert_array_equal(Ln[j:, :j], L[j + 1:, :j])
        np.testing.assert_array_equal(Wn[:j, :j], W[:j, :j])


def test_chunked_scan_equals_the_sequential_scan():
    """the order of the sums is all that differs: a few ε of the largest partial sum; and exactly equal on integers"""
    rng = np.random.default_rng(1)
    for n in (1, 63, 64, 65, 255, 256, 257, 700):
        v = rng.standard_normal(n)
        a, b = R.exclusive_scan(v, R.CHUNK), R.exclusive_scan(v, None)
        assert a[0] == 0.0 and np.max(np.abs(a - b)) <= 8 * EPS * np.sum(np.abs(v)), n
        vi = np.floor(rng.random(n) * 1000)
        np.testing.assert_array_equal(R.exclusive_scan(vi, R.CHUNK), R.exclusive_scan(vi, None))
    Kt, delta = _problem(300, seed=2)
    L, W, alpha, logdet, quad = R.refit(Kt, delta)
    for j in (0, 63, 64, 150, 299):
        a = R.remove(L, W, alpha, logdet, quad, j, R.CHUNK)
        b = R.remove(L, W, alpha, logdet, quad, j, None)
        bar = 16 * EPS * np.sqrt(np.linalg.cond(Kt))
        assert np.max(np.abs(a[0] - b[0])) <= bar and np.max(np.abs(a[1] - b[1])) <= bar * np.max(np.abs(W)), j
        assert a[3] == b[3] and a[4] == b[4]


def test_closed_forms_of_the_rank_one_factor():
    """C = chol(I + ppᵀ) and C⁻¹ as the header of csrc/remove.hip states them"""
    rng = np.random.default_rng(3)
    p = rng.standard_normal(40)
    rho = np.sqrt(1.0 + np.concatenate([[0.0], np.cumsum(p * p)]))
    m = len(p)
    Cm, Ci = np.zeros((m, m)), np.zeros((m, m))
    for k in range(m):
        Cm[k, k], Ci[k, k] = rho[k + 1] / rho[k], rho[k] / rho[k + 1]
        for i in range(k + 1, m):
            Cm[i, k] = p[i] * p[k] / (rho[k] * rho[k + 1])
            Ci[i, k] = -p[i] * p[k] / (rho[i] * rho[i + 1])
    assert np.max(np.abs(Cm @ Cm.T - (np.eye(m) + np.outer(p, p)))) <= 64 * EPS * rho[-1] ** 2
    assert np.max(np.abs(Ci @ Cm - np.eye(m))) <= 64 * EPS * rho[-1] ** 2


def test_scan_chunk_matches_the_kernels():
    src = open(os.path.join(ROOT, "abstractbayesopt.jl_amd", "csrc", "abo_kernels.h")).read()
    m = re.search(r"REMOVE_SCAN_CHUNK\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == 4 * R.CHUNK


def test_indices_are_sorted_and_checked():
    np.testing.assert_array_equal(incremental.remove_indices(5), [5])
    np.testing.assert_array_equal(incremental.remove_indices([7, 2, 5]), [2, 5, 7])
    np.testing.assert_array_equal(incremental.remove_indices(np.array([3, 1], dtype=np.int32)), [1, 3])
    assert incremental.remove_indices((4, 0)).dtype == np.int64
    with pytest.raises(ValueError, match="repeated"):
        incremental.remove_indices([3, 1, 3])
    with pytest.raises(ValueError, match="no index"):
        incremental.remove_indices([])
    for bad in (1.5, [1.0, 2.0], [True, False], "3"):
        with pytest.raises(TypeError):
            incremental.remove_indices(bad)


@pytest.mark.parametrize("make", [
    lambda: abo.HipGradientGP(abo.Matern52Kernel(), 3, 1e-3, device=0),
    lambda: abo.HipShardedGP(abo.Matern52Kernel(), 1e-3, devices=[0, 0]),
    lambda: abo.HipShardedGradientGP(abo.Matern52Kernel(), 3, 1e-3, devices=[0, 0]),
    lambda: object(),
])
def test_type_refusals(make):
    with pytest.raises(TypeError, match="remove_points"):
        abo.remove_points(make(), 0)


def test_unfitted_and_ard_models():
    with pytest.raises(ValueError, match="not conditioned"):
        abo.remove_points(abo.HipStandardGP(abo.Matern52Kernel(), 1e-3, device=0), 0)
    ard = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), (0.5, 2.0)), 1e-3, device=0)
    with pytest.raises(ValueError, match="not conditioned"):          # accepted as a type: it fails only for want of data
        abo.remove_points(ard, [1, 0])


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abo_hip.h")).read()
    assert re.search(r"^int32_t\s+abo_remove\s*\(", hdr, flags=re.M)
    assert "abo_remove" in abo._lib.EXPORTS and getattr(abo._lib.lib(), "abo_remove") is not None
    for path in (abo._lib.LIB_PATH, abo._lib.LIB_TEST_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert "abo_remove" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}, path
    for name, v in (("ABO_REMOVE_REMOVED", abo._lib.REMOVE_REMOVED), ("ABO_REMOVE_REFIT", abo._lib.REMOVE_REFIT)):
        assert re.search(rf"{name} = {v}\b", hdr), name
    assert abo._lib.REMOVE_PATHS == {0: "removed", 1: "refit"}
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr) and re.search(r"added within ABI 7.*abo_remove", hdr, flags=re.S)
    want = c_prototypes()["abo_remove"]
    assert want == [("abo_gp", 1), ("int64_t", 1), ("int32_t", 0), ("int32_t", 1), ("abo_gp", 2)]
    assert len(abo._lib.lib().abo_remove.argtypes) == len(want)
    from abstractbayesopt.jl_amd import build
    assert "remove.hip" in build.SOURCES


def test_argument_validation_needs_no_gpu():
    L = abo._lib.lib()
    idx = np.array([0], dtype=np.int64)
    out, path = C.c_void_p(), C.c_int32(-1)
    fake = C.c_void_p(0x1000)            # never dereferenced: every check below fails before the handle is looked at
    for gp, ip, k, op in ((None, idx.ctypes.data, 1, C.byref(out)), (fake, None, 1, C.byref(out)), (fake, idx.ctypes.data, 1, None),
                          (fake, idx.ctypes.data, 0, C.byref(out)), (fake, idx.ctypes.data, -2, C.byref(out))):
        path.value = -1
        assert L.abo_remove(gp, ip, k, C.byref(path), op) == abo._lib.ABO_EINVAL
        assert path.value == abo._lib.REMOVE_REFIT and "abo_remove" in abo._lib.last_error()
    assert out.value is None


def test_julia_shim_binds_remove_with_the_header_prototype():
    shim = os.path.join(ROOT, "integration", "julia", "RemovePoints.jl")
    calls = [c for c in julia_calls(shim) if c[0] == "abo_remove"]
    assert len(calls) == 1
    name, types, ret, line = calls[0]
    want = c_prototypes()[name]
    assert ret == "Int32" and len(types) == len(want)
    for jl, c in zip(types, want):
        assert jl_matches_c(jl, c), f"{shim}:{line}: {jl} vs {c}"
    main = open(os.path.join(ROOT, "integration", "julia", "HipStandardGP.jl")).read()
    assert 'include("RemovePoints.jl")' in main
    src = open(shim).read()
    assert ".- 1" in src and "sort!" in src               # 1-based in Julia, sorted for the library
