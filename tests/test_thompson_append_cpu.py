"""CPU tests of sample paths that follow the model through appends (include/abo_hip.h: abo_paths_append, _attach, _detach, _top,
_values, _append_stats_get): declaration, export and binding of the new names, argument checks that need no device, the host
methods' argument checking and `eps` bookkeeping with the library stubbed, the Julia bindings against the header — and the
block-inverse identity itself, restated twice in NumPy/SciPy:

  from scratch   the header's four formulas on the N + k points, `eps` extended by the k columns ε*:
                     v_s = K̃⁻¹(y − f_s(X) − σ_n·ε_s),   g_s(z) = f_s(z) + k(z, X)·v_s
  incremental    k times, with u = K̃⁻¹k(X, x*), s² = k(x*,x*) + σ²_n − k(X,x*)ᵀu:
                     a_s = (y* − σ_n·ε*_s − g_s(x*))/s²,   v'_s = [v_s − a_s·u; a_s],   g'_s(z) = g_s(z) + a_s·(k(z, x*) − k(z, X)·u)

Their largest disagreement over all paths and test candidates, in units of sqrt(σ_f²), is the δ the GPU tests' bars are built from
(tests/test_gpu_thompson_append.py imports `restate_scratch` / `restate_incremental` from here)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import thompson
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["abo_paths_append", "abo_paths_attach", "abo_paths_detach", "abo_paths_top", "abo_paths_values", "abo_paths_append_stats_get"]
JL = os.path.join(ROOT, "integration", "julia", "ThompsonAppend.jl")


def _features(hp, omega, phase, w, P):
    family, ell, sf2, noise, c = hp
    return c + w @ (math.sqrt(2.0 * sf2 / omega.shape[0]) * np.cos(P @ omega.T / ell + phase)).T


def restate_scratch(hp, X, y, base, Z, chunk=8192):
    """g (S, M) from scratch on all of (X, y): hp = (family, ℓ, σ_f², σ²_n, c), base = (omega, phase, w, eps (S × len(X)))"""
    family, ell, sf2, noise, c = hp
    omega, phase, w, eps = base
    K = O.kernel_matrix(family, ell, sf2, X, X)
    K[np.diag_indices_from(K)] += noise
    L = sla.cholesky(K, lower=True, overwrite_a=True, check_finite=False)
    V = sla.cho_solve((L, True), (y[None, :] - _features(hp, omega, phase, w, X) - math.sqrt(noise) * eps).T, check_finite=False)
    g = np.empty((w.shape[0], Z.shape[0]))
    for j0 in range(0, Z.shape[0], chunk):
        Zc = Z[j0:j0 + chunk]
        g[:, j0:j0 + chunk] = _features(hp, omega, phase, w, Zc) + (O.kernel_matrix(family, ell, sf2, Zc, X) @ V).T
    return g


def restate_incremental(hp, X, y, base, Z, k, chunk=8192):
    """the same paths by the incremental formulas: from scratch on the first len(X) − k points, then k one-point steps.  Returns
    (g (S, M), V (N + k, S)).  K̃⁻¹ of the growing model is applied through the base factor and the small Schur complement of the
    points appended so far (block elimination): no factorisation of the appended matrix is ever formed."""
    family, ell, sf2, noise, c = hp
    omega, phase, w, eps = base
    N0 = X.shape[0] - k
    X0 = X[:N0]
    K = O.kernel_matrix(family, ell, sf2, X0, X0)
    K[np.diag_indices_from(K)] += noise
    L0 = sla.cholesky(K, lower=True, overwrite_a=True, check_finite=False)
    sn = math.sqrt(noise)
    V = sla.cho_solve((L0, True), (y[None, :N0] - _features(hp, omega, phase, w, X0) - sn * eps[:, :N0]).T, check_finite=False)
    g = np.empty((w.shape[0], Z.shape[0]))
    for j0 in range(0, Z.shape[0], chunk):
        Zc = Z[j0:j0 + chunk]
        g[:, j0:j0 + chunk] = _features(hp, omega, phase, w, Zc) + (O.kernel_matrix(family, ell, sf2, Zc, X0) @ V).T
    W = np.empty((N0, 0))                                      # K̃₀⁻¹·k(X₀, appended points)
    for j in range(k):
        n = N0 + j
        xs, Xa = X[n:n + 1], X[N0:n]
        kx = O.kernel_matrix(family, ell, sf2, X[:n], xs)[:, 0]
        # u = K̃_n⁻¹ kx with K̃_n = [[K̃₀, B], [Bᵀ, Cc]]
        w1 = sla.cho_solve((L0, True), kx[:N0], check_finite=False)
        if j:
            B = O.kernel_matrix(family, ell, sf2, X0, Xa)
            Cc = O.kernel_matrix(family, ell, sf2, Xa, Xa) + noise * np.eye(j)
            x2 = np.linalg.solve(Cc - B.T @ W, kx[N0:] - B.T @ w1)
            u = np.concatenate([w1 - W @ x2, x2])
        else:
            u = w1
        s2 = sf2 + noise - kx @ u
        gx = _features(hp, omega, phase, w, xs)[:, 0] + kx @ V
        a = (y[n] - sn * eps[:, n] - gx) / s2
        for j0 in range(0, Z.shape[0], chunk):
            Zc = Z[j0:j0 + chunk]
            cz = O.kernel_matrix(family, ell, sf2, Zc, xs)[:, 0] - O.kernel_matrix(family, ell, sf2, Zc, X[:n]) @ u
            g[:, j0:j0 + chunk] += a[:, None] * cz[None, :]
        V = np.vstack([V - np.outer(u, a), a[None, :]])
        W = np.hstack([W, sla.cho_solve((L0, True), O.kernel_matrix(family, ell, sf2, X0, xs), check_finite=False)])
    return g, V


def delta_of(hp, g_scratch, g_inc):
    return float(np.max(np.abs(g_scratch - g_inc))) / math.sqrt(hp[2])


def test_new_names_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abo_hip.h")).read()
    lib = abo._lib.lib()
    for name in NAMES:
        assert re.search(r"^int32_t\s+%s\s*\(" % name, hdr, flags=re.M), f"{name} is not declared in the header"
        assert name in abo._lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, f"{name} has no argtypes"
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr)                       # new entry points only
    assert C.sizeof(abo._lib.AboPathsAppendStats) == 5 * 8
    assert C.sizeof(abo._lib.AboPathsStats) == 6 * 8                            # (the existing struct keeps its layout)
    assert "share their prior draw" in hdr
    for name in ("append", "attach", "detach", "top", "values", "append_stats"):
        assert callable(getattr(abo.SamplePaths, name))
    assert callable(abo.thompson_step)


def test_argument_validation_needs_no_device():
    lib, EINVAL = abo._lib.lib(), abo._lib.ABO_EINVAL
    buf = np.zeros(64)
    p, fake = buf.ctypes.data, C.c_void_p(buf.ctypes.data)
    assert lib.abo_paths_append(None, fake, p, 0) == EINVAL and "null" in abo._lib.last_error()
    assert lib.abo_paths_append(fake, None, p, 0) == EINVAL and "null" in abo._lib.last_error()
    assert lib.abo_paths_append(fake, fake, None, 0) == EINVAL and "null" in abo._lib.last_error()
    assert lib.abo_paths_append(fake, fake, p, 7) == EINVAL and "memory space" in abo._lib.last_error()
    assert lib.abo_paths_attach(None, fake) == EINVAL and lib.abo_paths_attach(fake, None) == EINVAL
    assert lib.abo_paths_detach(None) == EINVAL
    assert lib.abo_paths_top(None, 0, 1, p, p, 0) == EINVAL and lib.abo_paths_top(fake, 0, 1, None, p, 0) == EINVAL
    assert lib.abo_paths_top(fake, 0, 0, p, p, 0) == EINVAL and "k = 0" in abo._lib.last_error()
    assert lib.abo_paths_top(fake, 0, 1, p, p, 5) == EINVAL and "memory space" in abo._lib.last_error()
    assert lib.abo_paths_values(None, p, 0) == EINVAL and lib.abo_paths_values(fake, None, 0) == EINVAL
    assert lib.abo_paths_append_stats_get(None, None) == EINVAL


class _StubLib:
    """records the calls the host methods make; every call succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            return 0
        return f


def _stubbed_paths(monkeypatch, S=4, R=8, N=10, d=3):
    stub = _StubLib()
    monkeypatch.setattr(thompson, "_model_shape", lambda model: (N, d))
    monkeypatch.setattr(thompson._lib, "lib", lambda: stub)
    monkeypatch.setattr(abo.HipStandardGP, "_require", lambda self: 1234, raising=False)
    m = abo.HipStandardGP(abo.SqExponentialKernel(), 0.1)
    base = thompson.draw_base(abo.SqExponentialKernel(), S, R, N, d, 0)
    return stub, m, abo.SamplePaths(m, *base), base


def test_host_methods_check_their_arguments_and_keep_eps_consistent(monkeypatch):
    from abstractbayesopt.jl_amd.incremental import ResidentCandidates
    stub, m, paths, base = _stubbed_paths(monkeypatch)
    m2 = abo.HipStandardGP(abo.SqExponentialKernel(), 0.1)
    with pytest.raises(TypeError):
        paths.append(object())
    with pytest.raises(ValueError, match="S = 4"):
        paths.append(m2, np.zeros(5))
    with pytest.raises(ValueError, match="finite"):
        paths.append(m2, np.array([0.0, np.nan, 0.0, 0.0]))
    assert paths.eps.shape == (4, 10) and paths.model is m                       # refused steps leave the record alone
    e1 = np.array([0.1, -0.2, 0.3, -0.4])
    assert paths.append(m2, e1) is paths
    assert paths.eps.shape == (4, 11) and np.array_equal(paths.eps[:, 10], e1) and np.array_equal(paths.eps[:, :10], base[3])
    assert paths.model is m2 and paths.eps.flags["C_CONTIGUOUS"]
    assert stub.calls[-1][0] == "abo_paths_append"
    a = abo.SamplePaths.append(paths, m2, rng=5).eps[:, 11]
    assert np.array_equal(a, np.random.default_rng(5).standard_normal(4))        # drawn when not given, from the caller's seed
    for fn in (lambda: paths.top(), lambda: paths.values()):
        with pytest.raises(ValueError, match="attach"):
            fn()
    with pytest.raises(TypeError):
        paths.attach(np.zeros((3, 3)))
    cs = ResidentCandidates.__new__(ResidentCandidates)
    cs._h, cs.M, cs.d, cs.model = thompson._PathsHandle(None), 7, 3, m2
    paths.attach(cs)
    with pytest.raises(ValueError, match="already"):
        paths.attach(cs)
    with pytest.raises(ValueError, match="k = 0"):
        paths.top(0)
    tv, ti = paths.top(3, idx_base=5)
    assert tv.shape == (4, 3) and ti.shape == (4, 3) and ti.dtype == np.int64
    assert paths.values().shape == (4, 7)
    paths.detach()
    with pytest.raises(ValueError, match="attach"):
        paths.top()


def test_a_refused_append_leaves_the_python_record_untouched(monkeypatch):
    stub, m, paths, base = _stubbed_paths(monkeypatch)

    class Refusing(_StubLib):
        def __getattr__(self, name):
            if name == "abo_paths_append":
                return lambda *a: abo._lib.ABO_EINVAL
            if name == "abo_last_error":
                return lambda: b"refused"
            return super().__getattr__(name)
    monkeypatch.setattr(thompson._lib, "lib", lambda: Refusing())
    with pytest.raises(Exception):
        paths.append(abo.HipStandardGP(abo.SqExponentialKernel(), 0.1), np.zeros(4))
    assert paths.eps.shape == (4, 10) and paths.model is m


def test_julia_bindings_match_the_header():
    """integration/julia/ThompsonAppend.jl binds every new entry point; each call agrees with the header under the shim test's parser"""
    from tests import test_julia_shim_cpu as J
    protos = J.c_prototypes()
    calls = [c for c in J.julia_calls(JL) if c[0].startswith("abo_paths_")]
    assert {c[0] for c in calls} == set(NAMES)
    def matches(t, c):                                  # (the shim test's table of struct pointees predates the new struct)
        return J.jl_matches_c(t, c) or (t == "Ptr{AboPathsAppendStats}" and tuple(c) == ("abo_paths_append_stats", 1))
    for name, types, ret, line in calls:
        assert ret == "Int32" and len(types) == len(protos[name]), (name, line)
        assert all(matches(t, c) for t, c in zip(types, protos[name])), (name, line)
    jl = J.julia_struct(JL, "AboPathsAppendStats")
    cs = J.c_struct("abo_paths_append_stats")
    assert [f for f, _ in jl] == [f for f, _ in cs], (jl, cs)
    for (f, jt), (_, ct) in zip(jl, cs):
        assert J.SCALARS.get(jt) == ct, f"AboPathsAppendStats.{f}: {jt} against {ct}"
    assert 'include("ThompsonAppend.jl")' in open(J.SHIMS[0]).read()


def test_block_inverse_identity_incremental_equals_from_scratch():
    """Matérn-5/2, N = 50, d = 3, S = 16, R = 256, noise 1e-3, k = 8 appends, 400 candidates: the two restatements agree to rounding in
    path values and in v_s, with identical arg-mins on every path.  The bound is the identity's own: both routes are backward-stable
    fp64 solves of a system whose condition number κ ≤ (N + k)·σ_f²/σ²_n + 1, so they differ by at most a modest multiple of κ·ε."""
    fam, ell, sf2, noise, c, N, d, S, R, k = 1, 0.5, 1.4, 1e-3, 0.3, 50, 3, 16, 256, 8
    rng = np.random.default_rng(11)
    X = rng.random((N + k, d))
    y = np.sin(3.0 * X.sum(axis=1) / math.sqrt(d)) + 0.05 * rng.standard_normal(N + k)
    Z = rng.random((400, d))
    hp = (fam, ell, sf2, noise, c)
    base = thompson.draw_base(abo.Matern52Kernel(), S, R, N + k, d, rng)
    g1 = restate_scratch(hp, X, y, base, Z)
    g2, V2 = restate_incremental(hp, X, y, base, Z, k)
    K = O.kernel_matrix(fam, ell, sf2, X, X) + noise * np.eye(N + k)
    V1 = np.linalg.solve(K, (y[None, :] - _features(hp, base[0], base[1], base[2], X) - math.sqrt(noise) * base[3]).T)
    delta = delta_of(hp, g1, g2)
    relv = float(np.max(np.abs(V1 - V2)) / np.max(np.abs(V1)))
    print(f"block-inverse identity: delta = {delta:.3e} (path values / sqrt(sf2)), v_s relative {relv:.3e}; "
          f"a GPU case's bar = min(1e-6, max(100 * delta, 1e-12)) = {min(1e-6, max(100 * delta, 1e-12)):.3e}")
    kappa = (N + k) * sf2 / noise + 1.0
    assert delta <= 8.0 * kappa * np.finfo(float).eps
    assert relv <= 8.0 * kappa * np.finfo(float).eps
    assert np.array_equal(np.argmin(g1, axis=1), np.argmin(g2, axis=1))
    # and one step restated by hand against the library-independent formula g' = g + a·c
    g0 = restate_scratch(hp, X[:N], y[:N], (base[0], base[1], base[2], base[3][:, :N]), Z)
    g_one, _ = restate_incremental(hp, X[:N + 1], y[:N + 1], (base[0], base[1], base[2], base[3][:, :N + 1]), Z, 1)
    assert np.max(np.abs(g_one - g0)) > 1e-6                                       # (the step does move the paths)
    assert delta_of(hp, restate_scratch(hp, X[:N + 1], y[:N + 1], (base[0], base[1], base[2], base[3][:, :N + 1]), Z), g_one) \
        <= 8.0 * kappa * np.finfo(float).eps
