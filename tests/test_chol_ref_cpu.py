"""CPU tests of tests/chol_ref.py — the reference tests/test_gpu_chol_family.py holds the factorisation family to: the exact family is
exact (and LAPACK reproduces its factor bit for bit), LAPACK succeeds on every rung of the conditioning ladder, and the evaluators
of the backward-error measures see a zero residual as zero and one ulp as one ulp."""
import numpy as np
import pytest
import scipy.linalg as sla

from tests import chol_ref as R

SIZES = (128, 256, 528, 640, 1152, 1664)        # every size the GPU tests use (1664: the largest)


@pytest.mark.parametrize("n", SIZES)
def test_exact_family_is_exact_and_lapack_reproduces_it(n):
    A, L0, W0 = R.exact_case(n, seed=n)
    worst = R.assert_exact(L0, W0)
    assert worst < 2 ** 53 // 2 ** 20                          # (far below: not a near miss)
    assert np.all(A == np.rint(A)) and A.min() < 0 and np.array_equal(A, A.T)
    assert np.array_equal(np.triu(L0, 1), np.zeros((n, n))) and np.array_equal(np.triu(W0, 1), np.zeros((n, n)))
    # pivots are powers of four, pair determinants too
    d = np.diag(L0) ** 2
    assert np.all(np.log2(d) % 2 == 0)
    assert np.array_equal(np.linalg.cholesky(A), L0)
    # E is non-zero only at (odd row, even column): the structure E² = 0 rests on
    off = L0 - np.diag(np.diag(L0))
    i, j = np.nonzero(off)
    assert len(i) > n and np.all(i % 2 == 1) and np.all(j % 2 == 0)


def test_signed_family_is_signed_and_well_conditioned():
    for n in (128, 528, 640):
        A = R.signed_spd(n, seed=n)
        assert A.min() < 0 and np.array_equal(A, A.T)
        assert np.linalg.cond(A) < 10.0


@pytest.mark.parametrize("n", [528, 640])          # the two sizes the GPU tests take ladder matrices at
def test_lapack_succeeds_on_every_rung_of_the_ladder(n):
    cases = R.ladder_cases(n)
    assert len(cases) == len(R.LADDER_FAMILIES) * len(R.NOISES)
    kaps = []
    for name, A, kap in cases:
        assert f"{kap:.1e}" in name
        L = np.linalg.cholesky(A)                              # raises LinAlgError on a failing pivot
        assert np.all(np.isfinite(L)) and np.all(np.diag(L) > 0)
        # LAPACK's own backward error is at the rounding level on every rung, whatever κ₂
        e, r = R.backward(A, L)
        assert e < 64 * R.U and r < R.gamma(n + 1)
        kaps.append(kap)
    # the ladder climbs: each family's rungs are ordered, the top one beyond 1e10
    for f in range(len(R.LADDER_FAMILIES)):
        k = kaps[f * len(R.NOISES):(f + 1) * len(R.NOISES)]
        assert all(a < b for a, b in zip(k, k[1:])) and k[-1] > 1e10


@pytest.mark.parametrize("n", [128, 640, 1152])
def test_measures_on_the_exact_family_and_one_ulp(n):
    """the residual of the exact family is exactly zero under both evaluators (long double up to 640, sliced above); one ulp on one
    entry L[i][j] changes (A − LLᵀ) by −ulp·L[k][j] in row/column i — the known change — and nothing elsewhere"""
    A, L0, W0 = R.exact_case(n, seed=n)
    assert R.eta(A, L0) == 0.0 and R.rho(A, L0) == 0.0 and R.inv_res(L0, W0) == 0.0
    assert not np.any(R.resid_sliced(A, L0, L0)) and not np.any(R.resid_sliced(np.eye(n), W0, np.ascontiguousarray(L0.T)))
    i, j = n - 3, n - 4                                        # (odd row, even column) or the other way round: any entry will do
    L = L0.copy()
    L[i, j] = 3.0
    h = np.spacing(3.0)
    L[i, j] += h
    A3 = L0.copy()
    A3[i, j] = 3.0
    A3 = A3 @ A3.T                                             # exact, as A is
    for ev in (R.resid, R.resid_sliced):
        D = ev(A3, L, L)
        want = np.zeros((n, n))
        want[i, :] -= h * L[:, j]
        want[:, i] -= h * L[:, j]
        want[i, i] = -(2 * 3.0 * h + h * h)
        assert np.max(np.abs(D - want)) <= 2.0 ** -10 * h, ev.__name__
    e = R.eta(A3, L)
    assert abs(e - np.max(np.abs(want)) / np.max(np.abs(A3))) <= 2.0 ** -10 * e
    # the inverse: one ulp on W[i][i] leaves (WL − I)[i][i] = ulp·L[i][i]
    W = W0.copy()
    hw = np.spacing(W[i, i])
    W[i, i] += hw
    got = R.inv_res(L0, W)
    den = (np.abs(W) @ np.abs(L0))[i, i]
    assert abs(got - hw * L0[i, i] / den) <= 2.0 ** -10 * got


def test_sliced_products_agree_with_long_double_on_rounded_data():
    if not R.HAVE_LD:
        pytest.skip("long double is fp64 here: the sliced evaluator stands alone")
    A = R.ladder_matrix(R.LADDER_FAMILIES[0], 1e-8, 256)
    L = np.linalg.cholesky(A)
    a, b = R.resid(A, L, L), R.resid_sliced(A, L, L)
    # 2¹⁰ below what they measure (the long double product's own error, ≈ √n·2⁻⁶⁴ of the scale, is the larger of the two)
    assert np.max(np.abs(a)) > 0 and np.max(np.abs(a - b)) <= 2.0 ** -10 * np.max(np.abs(a))


def test_kappa16_and_the_panel_residual():
    A = R.signed_spd(144, seed=3)
    L = np.linalg.cholesky(A)
    assert R.kappa16(L) == max(np.linalg.cond(L[o:o + 16, o:o + 16]) for o in range(0, 144, 16))
    Lbb = L[:128, :128]
    X = sla.solve_triangular(Lbb, A[128:, :128].T, lower=True).T
    assert R.panel_res(A[128:, :128], X, Lbb) < 64 * R.U
    assert R.gamma(10) == pytest.approx(10 * R.U) and R.inv_bar(2.0) == 32 * R.U
    assert np.array_equal(R.ulp_diff(np.array([1.0 + 2 ** -52]), np.array([1.0])), [1.0])
