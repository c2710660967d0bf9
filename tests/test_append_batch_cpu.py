"""CPU tests of abo_append_batch / append_points (no GPU needed): the identities of the blocked bordered step restated in NumPy
(tests/append_batch_oracle.py) against dense refits and against k sequential one-row steps, at the bars tests/test_remove_cpu.py holds
its closed forms to; the argument handling of append_points; the C-ABI declared, exported, bound by _lib.py and the Julia shim with
the header's prototype, and refusing bad arguments before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import incremental
from tests import append_batch_oracle as A
from tests.test_julia_shim_cpu import c_prototypes, jl_matches_c, julia_calls
from tests.test_remove_cpu import EPS, _bars, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(N, k) for N in (1, 7, 130) for k in (1, 2, 16, 33, 64)]


def _split(N, k):
    Kt, delta = _problem(N + k, seed=N * 100 + k)
    return Kt, delta, A.refit(Kt[:N, :N], delta[:N])


def _agree(a, b, Kt, what):
    """two factor states of the same K̃ at test_remove_cpu's bars (b: the reference)"""
    bar_L, bar_inv = _bars(Kt)
    n = Kt.shape[0]
    La, Wa, aa, lda, qa = a
    Lb, Wb, ab, ldb, qb = b
    assert np.max(np.abs(La - Lb)) <= bar_L, what
    assert np.max(np.abs(np.triu(La, 1))) == 0.0 and np.max(np.abs(np.triu(Wa, 1))) == 0.0, what
    assert np.max(np.abs(Wa @ Lb - np.eye(n))) <= bar_inv, what
    assert np.max(np.abs(aa - ab)) / np.max(np.abs(ab)) <= bar_inv, what
    assert abs(lda - ldb) <= bar_inv * n and abs(qa - qb) / abs(qb) <= bar_inv, what


@pytest.mark.parametrize("N,k", SHAPES)
def test_blocked_step_matches_the_dense_refit(N, k):
    Kt, delta, st = _split(N, k)
    new = A.append_batch(*st, Kt[:N, N:], Kt[N:, N:], delta[N:])
    _agree(new, A.refit(Kt, delta), Kt, (N, k))
    # the old rows are copies, bit for bit
    np.testing.assert_array_equal(new[0][:N, :N], st[0])
    np.testing.assert_array_equal(new[1][:N, :N], st[1])


@pytest.mark.parametrize("N,k", SHAPES)
def test_blocked_step_matches_sequential_steps(N, k):
    Kt, delta, st = _split(N, k)
    blocked = A.append_batch(*st, Kt[:N, N:], Kt[N:, N:], delta[N:])
    seq = A.append_sequential(*st, Kt, delta, N, k)
    _agree(blocked, seq, Kt, (N, k))
    _agree(seq, A.refit(Kt, delta), Kt, (N, k))


def test_failing_pivot_is_reported_in_refit_order():
    """a repeated row with no noise makes its pivot exactly zero: pivot j of S is what a refit's potrf reports as N + j + 1"""
    S = np.eye(6)
    S[1, 3] = S[3, 1] = 1.0                                           # row 3 repeats row 1
    assert A.pivot_of(S) == 3
    S[4, 4] = -1.0
    assert A.pivot_of(S) == 3                                         # the FIRST failing pivot
    assert A.pivot_of(np.eye(4)) == -1
    Kt, delta, st = _split(7, 6)
    Kbb = Kt[7:, 7:].copy()
    Kbb[3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        A.append_batch(*st, Kt[:7, 7:], Kbb, delta[7:])


@pytest.mark.parametrize("make", [
    lambda: abo.HipGradientGP(abo.Matern52Kernel(), 3, 1e-3, device=0),
    lambda: abo.HipShardedGP(abo.Matern52Kernel(), 1e-3, devices=[0, 0]),
    lambda: abo.HipShardedGradientGP(abo.Matern52Kernel(), 3, 1e-3, devices=[0, 0]),
    lambda: object(),
])
def test_type_refusals(make):
    with pytest.raises(TypeError, match="append_points"):
        abo.append_points(make(), np.zeros((2, 2)), np.zeros(2))


def test_argument_refusals():
    m = abo.HipStandardGP(abo.Matern52Kernel(), 1e-3, device=0)
    with pytest.raises(ValueError, match="empty"):
        abo.append_points(m, np.zeros((0, 3)), np.zeros(0))
    with pytest.raises(abo._lib.DimensionMismatch, match="3 points but 2 targets"):
        abo.append_points(m, np.zeros((3, 2)), np.zeros(2))
    with pytest.raises(abo._lib.DimensionMismatch):
        abo.append_points(m, [[0.0, 1.0], [2.0]], np.zeros(2))            # ragged
    with pytest.raises(ValueError, match="not conditioned"):              # accepted as arguments: it fails only for want of data
        abo.append_points(m, np.zeros((3, 2)), np.zeros(3))
    ard = abo.HipStandardGP(abo.with_lengthscale(abo.Matern52Kernel(), (0.5, 2.0)), 1e-3, device=0)
    with pytest.raises(abo.ArdUnsupported, match="append_points"):
        abo.append_points(ard, np.zeros((3, 2)), np.zeros(3))
    xp, k, d, yp, space, keep = incremental.batch_points([[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]], [1, 2, 3])
    assert (k, d, space) == (3, 2, abo._lib.HOST)
    assert abo.append_points is incremental.append_points


def test_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "abo_hip.h")).read()
    assert re.search(r"^int32_t\s+abo_append_batch\s*\(", hdr, flags=re.M)
    assert "abo_append_batch" in abo._lib.EXPORTS and getattr(abo._lib.lib(), "abo_append_batch") is not None
    assert "abo_test_tri_skinny" in abo._lib.TEST_EXPORTS and "abo_test_tri_skinny" not in abo._lib.EXPORTS
    syms = {}
    for path in (abo._lib.LIB_PATH, abo._lib.LIB_TEST_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        syms[path] = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert "abo_append_batch" in syms[path], path
    assert "abo_test_tri_skinny" in syms[abo._lib.LIB_TEST_PATH] and "abo_test_tri_skinny" not in syms[abo._lib.LIB_PATH]
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr) and re.search(r"added within ABI 7.*abo_append_batch", hdr, flags=re.S)
    assert abo._lib.ABI_VERSION == 7
    want = c_prototypes()["abo_append_batch"]
    assert want == [("abo_gp", 1), ("double", 1), ("int32_t", 0), ("int32_t", 0), ("double", 1), ("int32_t", 0), ("int64_t", 1),
                    ("abo_gp", 2)]
    assert len(abo._lib.lib().abo_append_batch.argtypes) == len(want)
    hook = re.search(r"\bint32_t\s+abo_test_tri_skinny\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
    assert hook and hdr.index("#ifdef ABO_TEST_HOOKS") < hook.start() < hdr.index("#endif /* ABO_TEST_HOOKS */")
    from abstractbayesopt.jl_amd import build
    assert "append_batch.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "abstractbayesopt.jl_amd", "csrc", "abo_kernels.h")).read()
    assert re.search(r"APPEND_BATCH_MAX\s*=\s*64\b", src)


def test_argument_validation_needs_no_gpu():
    L = abo._lib.lib()
    x, y = np.zeros((2, 3)), np.zeros(2)
    out, info = C.c_void_p(), C.c_int64(-1)
    fake = C.c_void_p(0x1000)            # never dereferenced: every check below fails before the handle is looked at
    for gp, xp, k, yp, op in ((None, x.ctypes.data, 2, y.ctypes.data, C.byref(out)), (fake, None, 2, y.ctypes.data, C.byref(out)),
                              (fake, x.ctypes.data, 2, None, C.byref(out)), (fake, x.ctypes.data, 2, y.ctypes.data, None),
                              (fake, x.ctypes.data, 0, y.ctypes.data, C.byref(out)), (fake, x.ctypes.data, -3, y.ctypes.data, C.byref(out))):
        info.value = -1
        assert L.abo_append_batch(gp, xp, k, 3, yp, abo._lib.HOST, C.byref(info), op) == abo._lib.ABO_EINVAL
        assert info.value == 0 and "abo_append_batch" in abo._lib.last_error()
    assert out.value is None


def test_julia_shim_binds_append_batch_with_the_header_prototype():
    shim = os.path.join(ROOT, "integration", "julia", "AppendPoints.jl")
    calls = [c for c in julia_calls(shim) if c[0] == "abo_append_batch"]
    assert len(calls) == 1
    name, types, ret, line = calls[0]
    want = c_prototypes()[name]
    assert ret == "Int32" and len(types) == len(want)
    for jl, c in zip(types, want):
        assert jl_matches_c(jl, c), f"{shim}:{line}: {jl} vs {c}"
    main = open(os.path.join(ROOT, "integration", "julia", "HipStandardGP.jl")).read()
    assert 'include("AppendPoints.jl")' in main
    assert "`abo_append_batch`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
