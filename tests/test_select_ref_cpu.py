"""The references of tests/test_gpu_select_family.py (tests/select_ref.py) checked on their own, no GPU needed: a reference that is
wrong in a corner would make the GPU file assert the wrong thing there."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import gp_oracle as O

from tests import select_ref as R

NAN = float("nan")
INF = float("inf")


def test_sortperm_rev_on_a_hand_written_case():
    """both NaNs, both infinities, both zeros, a subnormal and a tie; the order written out by hand from Julia's isless:
    NaN (index order, whatever sign or payload) > +Inf > 2.5 (twice: index order) > 5e-324 > 0.0 > −0.0 > −1.0 > −Inf"""
    s = np.array([-1.0, R.nan_with(1, 7), 0.0, INF, -0.0, 2.5, 5e-324, -INF, 2.5, R.nan_with(0, 1 << 51), -0.0, 0.0])
    want = [1, 9, 3, 5, 8, 6, 2, 11, 4, 10, 0, 7]
    assert R.sortperm_rev(s, 12).tolist() == want
    assert R.sortperm_rev(s, 40).tolist() == want
    assert R.sortperm_rev(s, 5).tolist() == want[:5]
    assert R.sortperm_rev(s, 0).tolist() == []
    idx, val = R.topk_expect(s, 12, 14, 2 ** 33 + 5)
    assert idx.tolist() == [w + 2 ** 33 + 5 for w in want] + [-1, -1]
    assert val[0] == R.bits(s)[1] and val[1] == R.bits(s)[9] and val[0] != val[1]          # the payloads, not a canonical NaN
    assert val[12] == R.QNAN_BITS and val[13] == R.QNAN_BITS
    assert (val[6], val[8]) == (np.uint64(0), np.uint64(1 << 63))                          # 0.0 then −0.0, told apart by their bits
    idx, val = R.topk_expect(s, 0, 3, 0)                                                   # an empty batch
    assert idx.tolist() == [-1, -1, -1] and (val == R.QNAN_BITS).all()


@pytest.mark.parametrize("n", [1, 2, 17, 1000])
def test_sortperm_rev_does_not_depend_on_the_order_of_tie_free_data(n):
    rng = np.random.default_rng(n)
    s = rng.standard_normal(n)
    big = np.finfo(np.float64).max
    sp = np.array([INF, -INF, 5e-324, -5e-324, big, -big, 0.0])[: n // 5]                       # tie-free still: one zero only
    s[: sp.size] = sp
    assert np.unique(s).size == n
    ref = R.sortperm_rev(s, n)
    assert np.all(np.diff(s[ref]) < 0)
    for _ in range(3):
        perm = rng.permutation(n)
        assert np.array_equal(perm[R.sortperm_rev(s[perm], n)], ref)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M", [1, 2, 63, 1025, 5000])
def test_sortperm_rev_agrees_with_the_oracle(fam, M):
    """the two are written differently (the oracle folds NaN into +Inf with a rank of its own); since the oracle learnt the ±0 rule
    they agree on every family, −0.0 included"""
    s = R.scores_family(fam, M, seed=3)
    for k in (1, 2, M, M + 3):
        ov, oi = O.top_k(s, k)
        got = R.sortperm_rev(s, k)
        assert np.array_equal(got, oi)
        assert np.array_equal(R.bits(ov), R.bits(s)[got])


def test_oracle_top_k_ranks_positive_zero_first():
    s = np.array([-0.0, 0.0, -1.0, 0.0, -0.0, NAN])
    assert O.top_k(s, 6)[1].tolist() == [5, 1, 3, 0, 4, 2]
    assert R.sortperm_rev(s, 6).tolist() == [5, 1, 3, 0, 4, 2]


def test_score_families_are_what_the_gpu_file_says_they_are():
    M = 5000
    assert np.unique(R.scores_family("b", M, 1)).size == 3
    assert np.unique(R.scores_family("c", M, 1)).size == 1
    d = R.scores_family("d", M, 1)
    assert np.isnan(d).all() and np.signbit(d).any() and not np.signbit(d).all() and np.unique(R.bits(d)).size > M // 2
    e = R.scores_family("e", M, 1)
    for place, v in zip(R.special_places(M), R.SPECIALS):
        assert R.bits(e)[place] == R.bits(np.array([v]))[0]
    assert R.special_places(M)[0] == 0 and R.special_places(M)[-1] == M - 1
    f = R.bits(R.scores_family("f", M, 1))
    assert np.unique(f >> np.uint64(8)).size == 1 and np.unique(f & np.uint64(0xff)).size == 256
    assert (R.scores_family("g", M, 1) < 0).all()
    for fam in R.FAMILIES:
        assert np.array_equal(R.bits(R.scores_family(fam, 77, 5)), R.bits(R.scores_family(fam, 77, 5)))      # seeded


def test_prune_keep_ref_corner_cases():
    a = 2.0 ** -1022
    ub = np.array([NAN, INF, -INF, 1.0, -1.0, 0.0])
    assert R.prune_keep_ref(ub, 0.5, a).tolist() == [True, True, True, True, False, False]       # −Inf + Inf = NaN: kept
    assert R.prune_keep_ref(ub, NAN, a).all()
    assert R.prune_keep_ref(ub, -INF, a).all()
    assert R.prune_keep_ref(ub, INF, a).tolist() == [True, True, True, False, False, False]
    assert R.prune_keep_ref(np.array([0.0]), 2.0 ** -30, 2.0 ** -30).tolist() == [True]           # the absolute margin alone
    assert R.prune_keep_ref(np.array([0.0]), 2.0 ** -30, a).tolist() == [False]


@pytest.mark.parametrize("tau", [0.3, -0.3, 7.25e-3, 123.456])
@pytest.mark.parametrize("abs_margin", [2.0 ** -1022, 2.0 ** -30])
def test_guard_boundary_straddles_the_threshold(tau, abs_margin):
    b = R.guard_boundary(tau, abs_margin)
    keep = R.prune_keep_ref(b, tau, abs_margin)
    assert np.all(np.diff(b) > 0) and not keep[0] and keep[-1]                                    # both sides, one ulp apart
    assert np.all(np.diff(keep.astype(int)) >= 0)


def test_finalize_ref_against_a_scalar_loop():
    rng = np.random.default_rng(0)
    T, Mc, j0, M = 3, 16, 5, 18
    partial, mu_in = rng.uniform(0, 0.1, size=(T, Mc)), rng.standard_normal(Mc)
    tail, eps, head, ssq = rng.standard_normal(M + 2), rng.uniform(0, 1e-3, M + 2), rng.standard_normal(M + 2), rng.uniform(0, 0.1, M + 2)
    mu, var, tl = R.finalize_ref(partial, mu_in, M, j0, Mc, T, 1.5, prior_grad=0.25, pc=3, point_major=1, mu_tail=tail, mu_eps=eps,
                                 head_g=head, ssq_g=ssq)
    for gj in range(M + 2):
        if gj < j0 or gj >= M:
            assert np.isnan(mu[gj]) and np.isnan(var[gj]) and tl[gj] == tail[gj]
            continue
        q = ssq[gj]
        for t in range(T):
            q += partial[t, gj - j0]
        m = head[gj] + tail[gj]
        assert var[gj] == ((1.5 if gj % 3 == 0 else 0.25) - q) + 1e-18 and tl[gj] == m and mu[gj] == m - eps[gj]
    mu, var, tl = R.finalize_ref(partial, mu_in, M, j0, Mc, T, 1.5, prior_grad=0.25, pc=2, point_major=0, Mpts=9)
    assert tl is None and mu[j0] == mu_in[0]
    assert var[8] == (1.5 - ((partial[0, 3] + partial[1, 3]) + partial[2, 3])) + 1e-18
    assert var[9] == (0.25 - ((partial[0, 4] + partial[1, 4]) + partial[2, 4])) + 1e-18


def test_guarded_keeps_an_infinite_score():
    g = R.guarded(np.array([1.0, -1.0, 0.0, INF, -INF]), 2.0 ** -30)
    assert g.tolist() == [1.0 + 2.0 ** -29, -1.0 + 2.0 ** -29, 2.0 ** -30, INF, -INF]


def test_fma_ref_rounds_once_on_the_operands_of_the_downdate_test():
    """exact rationals: the long double sum of downdate_operands() is the true value, so fma_ref is the correctly rounded fma — and on
    a good part of the operands a multiply followed by an add gives another result, which is what the GPU test can then tell apart"""
    c, beta, mu, _, _ = R.downdate_operands(2000, seed=1)
    ref = R.fma_ref(c, beta, mu)
    differs = 0
    for cj, mj, rj in zip(c, mu, ref):
        exact = Fraction(float(cj)) * Fraction(beta) + Fraction(float(mj))
        assert rj == float(exact)                             # int / int: correctly rounded
        differs += rj != cj * beta + mj
    assert differs > 100


def test_gradnorm_ref_against_the_formula():
    m = np.array([9.0, 1.0, -2.0])
    Cm = np.array([[7.0, 0.0, 0.0], [0.0, 2.0, 0.5], [0.0, 0.5, 1.0]])
    # mm = 5, tr = 3, msm = 1·(2 − 1) − 2·(0.5 − 2) = 4, fro = 4 + 0.25 + 0.25 + 1 = 5.5
    score, bar = R.gradnorm_ref(m, Cm, 2.0)
    assert abs(score - (-8.0 + 2.0 * np.sqrt(27.0))) < 1e-15 and 0 < bar < 1e-13
    score, _ = R.gradnorm_ref(np.zeros(3), np.zeros((3, 3)), 3.0)
    assert abs(score - 3.0e-6) < 1e-20                        # the floor 1e-12 under the root
