"""Exact top-k without the full variance contraction (csrc/acq.hip: prune_select; DESIGN.md "Pruned top-k selection").

A call that asks for the top k only (EI, or UCB with β ≥ 0, int8-residue engine) bounds every score from above with the variance
reduction of the first rows of L⁻¹ alone, takes a threshold from the exact scores of the best-by-bound candidates and runs the full
contraction only on the candidates whose bound reaches it.  Every case compares that call with the same call with the path switched
off (abo_test_prune_force mode 2 = ABO_ACQ_PRUNE=0) and asks for EXACT equality of the k values and the k indices; the selection is
also checked against the oracle: indices = O.top_k of the library's full score vector, values = the oracle's scores there at the
tolerance of tests/test_gpu_parity.py (rtol 1e-6, atol 1e-12)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

from tests.test_gpu_parity import make_model

ELL, SF2, NOISE, XI, BETA = 1.0, 1.0, 1e-3, 0.01, 2.0
PRUNE_REL, PRUNE_ABS = 2.0 ** -30, 2.0 ** -1022          # csrc/abo_kernels.h


def _force(rblocks, mode):
    abo._lib.check(abo._lib.lib().abo_test_prune_force(rblocks, mode))


@pytest.fixture(autouse=True)
def _defaults():
    _force(0, 0)
    yield
    _force(0, 0)


def _acq(name, y):
    return abo.ExpectedImprovement(XI, float(np.min(y))) if name == "ei" else abo.UpperConfidenceBound(BETA)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _both(acq, model, Z, k, idx_base=0):
    """(values, indices, statistics) of the pruned call, after asserting that the call with the path off returns the same bits"""
    _, tv, ti = abo.evaluate(acq, model, Z, k=k, idx_base=idx_base, return_scores=False)
    st = model.prune_stats()
    _force(0, 2)
    _, tv0, ti0 = abo.evaluate(acq, model, Z, k=k, idx_base=idx_base, return_scores=False)
    st0 = model.prune_stats()
    _force(0, 0)
    assert st0["bound_rows"] == 0 and st0["pruned"] == 0 and st0["fallback"] == 0
    np.testing.assert_array_equal(ti, ti0)
    np.testing.assert_array_equal(_bits(tv), _bits(tv0))
    return tv, ti, st


def _against_oracle(kind, acq, model, X, y, Z, k, tv, ti, idx_base=0):
    s, _, _ = abo.evaluate(acq, model, Z, k=0)
    assert model.prune_stats()["bound_rows"] == 0                    # a call that returns scores runs the full pass
    ov, oi = O.top_k(s, k)
    np.testing.assert_array_equal(ti, oi + idx_base)
    st = O.fit(O.MATERN52, ELL, SF2, NOISE, 0.0, X, y)
    mu, var = O.predict(st, Z)
    ref = O.acquisition(kind, mu, var, acq._p0(), acq._best())
    sel = ti[ti >= 0] - idx_base
    np.testing.assert_allclose(tv[ti >= 0], ref[sel], rtol=1e-6, atol=1e-12)
    return s


@pytest.fixture(scope="module")
def typical():
    N, d, M = 1536, 8, 20000                                          # six row blocks of L⁻¹
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(O.MATERN52, ELL, SF2, NOISE, contraction="int8"), X, y)
    return X, y, Z, model


@pytest.mark.parametrize("name,kind", [("ei", O.ACQ_EI), ("ucb", O.ACQ_UCB)])
def test_typical_case_prunes_and_bounds_dominate(typical, name, kind):
    X, y, Z, model = typical
    M, k = Z.shape[0], 100
    acq = _acq(name, y)
    tv, ti, st = _both(acq, model, Z, k)
    print(f"{name}: {st}")
    assert st["pruned"] == 1 and st["fallback"] == 0 and st["bound_rows"] == 256 and st["k0"] == 1024
    assert k <= st["survivors"] < M // 2
    assert model.timings()["contraction_engine"] == abo._lib.CONTRACT_INT8
    # bound dominance: the guarded bound of every candidate is at least its exact score
    abo.evaluate(acq, model, Z, k=k, return_scores=False)
    ub = np.empty(M)
    abo._lib.check(abo._lib.lib().abo_test_prune_bounds(model._require(), ub.ctypes.data, M))
    s = _against_oracle(kind, acq, model, X, y, Z, k, tv, ti)
    slack = ub * (1.0 + PRUNE_REL) + PRUNE_ABS - s
    print(f"{name}: min(guarded bound - score) = {slack.min():.3e}, bound > score on {np.mean(ub > s):.4f} of the candidates")
    assert np.all(slack >= 0.0)


def test_ragged_sizes_and_index_base():
    N, d, M, k, base = 1300, 8, 5000, 100, 123456789                  # ragged last row block, M no multiple of 256
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(O.MATERN52, ELL, SF2, NOISE, contraction="int8"), X, y)
    acq = _acq("ei", y)
    tv, ti, st = _both(acq, model, Z, k, idx_base=base)
    print(st)
    assert st["pruned"] == 1 and st["bound_rows"] == 256
    assert ti.min() >= base
    _against_oracle(O.ACQ_EI, acq, model, X, y, Z, k, tv, ti, idx_base=base)


@pytest.fixture(scope="module")
def small():
    N, d = 1300, 8
    X, y = synth.standardized_problem(N, d, 0.03)
    model = abo.update(make_model(O.MATERN52, ELL, SF2, NOISE, contraction="int8"), X, y)
    return X, y, model


def test_ties_across_the_threshold_keep_index_order(small):
    X, y, model = small
    M, k = 5000, 100
    Z = synth.points(2, 625, 8)[np.arange(M) % 625]                   # every point 8 times: ranks 97-104 hold one score, k = 100 cuts it
    acq = _acq("ei", y)
    tv, ti, st = _both(acq, model, Z, k)
    print(st)
    assert st["pruned"] == 1
    s = _against_oracle(O.ACQ_EI, acq, model, X, y, Z, k, tv, ti)
    assert np.sum(s == tv[k - 1]) > np.sum(tv == tv[k - 1]) >= 1      # more candidates hold the k-th score than were selected


def test_nan_candidate_is_ranked_as_the_full_path_ranks_it(small):
    X, y, model = small
    M, k = 5000, 100
    Z = synth.points(2, M, 8).copy()
    Z[1234, 3] = np.nan
    Z[4999, 0] = np.nan
    for name in ("ei", "ucb"):
        acq = _acq(name, y)
        tv, ti, st = _both(acq, model, Z, k)
        print(name, st)
        assert st["bound_rows"] == 256
        assert list(ti[:2]) == [1234, 4999] and np.isnan(tv[:2]).all() and not np.isnan(tv[2:]).any()


def test_degenerate_sizes(small):
    X, y, model = small
    acq = _acq("ei", y)
    Z = synth.points(2, 5000, 8)
    tv, ti, st = _both(acq, model, Z, 1)                              # k = 1: K0 = 1024
    print(st)
    assert st["pruned"] == 1 and st["k0"] == 1024
    _against_oracle(O.ACQ_EI, acq, model, X, y, Z, 1, tv, ti)
    tv, ti, st = _both(acq, model, Z[:50], 100)                       # k ≥ M: below the floor, the full pass; tail (NaN, −1)
    assert st["bound_rows"] == 0
    assert np.all(ti[50:] == -1) and np.isnan(tv[50:]).all() and sorted(ti[:50]) == list(range(50))


def test_nothing_prunable_takes_the_fallback():
    N, d, M, k = 1300, 8, 5000, 100
    X = synth.points(1, N, d)
    y = np.full(N, 0.5)
    Z = synth.points(2, M, d) + 1000.0                                # far from the data: every bound and every score is the prior's
    model = abo.update(make_model(O.MATERN52, ELL, SF2, NOISE, contraction="int8"), X, y)
    for name in ("ei", "ucb"):
        acq = _acq(name, y)
        tv, ti, st = _both(acq, model, Z, k)
        print(name, st)
        assert st["fallback"] == 1 and st["pruned"] == 0 and st["survivors"] == M and st["bound_rows"] == 256
        np.testing.assert_array_equal(ti, np.arange(k))
        # the timings count the bound pass and the threshold pass next to the full pass
        abo.evaluate(acq, model, Z, k=k, return_scores=False)
        t = model.timings()
        assert t["var_gemm_flop"] == 256.0 ** 2 * M + float(N) ** 2 * (1024 + M)


def test_calls_that_are_not_eligible_run_the_full_pass(typical):
    X, y, Z, model = typical
    k = 100
    abo.evaluate(abo.ProbabilityImprovement(XI, float(np.min(y))), model, Z, k=k, return_scores=False)
    assert model.prune_stats() == {"pruned": 0, "fallback": 0, "bound_rows": 0, "k0": 0, "survivors": 0, "bound_ms": 0.0,
                                   "threshold_ms": 0.0, "survivor_ms": 0.0}
    abo.evaluate(_acq("ei", y), model, Z, k=k, return_scores=True)
    assert model.prune_stats()["bound_rows"] == 0
    abo.evaluate(abo.UpperConfidenceBound(-1.0), model, Z, k=k, return_scores=False)
    assert model.prune_stats()["bound_rows"] == 0
    m64 = abo.update(make_model(O.MATERN52, ELL, SF2, NOISE, contraction="fp64"), X, y)      # the fp64 engine is left out
    _, tv64, ti64 = abo.evaluate(_acq("ei", y), m64, Z, k=k, return_scores=False)
    assert m64.prune_stats()["bound_rows"] == 0 and m64.timings()["contraction_engine"] == abo._lib.CONTRACT_FP64
