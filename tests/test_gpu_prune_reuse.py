"""Survivors that the threshold pass of the pruned top-k selection has scored are not evaluated again (csrc/acq.hip: prune_select,
prune_survivors; csrc/misc.hip: prune_reuse_kernel).  int8 engine, k = 100 (K₀ = 1024); every selection is asked to equal, bit
for bit, the same call with the path off (abo_test_prune_force(0, 2)) and with the switch off (ABO_PRUNE_REUSE=0 through its hook).

  * N = 3072, M = 20 000, EI and UCB(2): both calls reuse (their survivors are fewer than K₀), same survivor count either way;
  * ties: 50 copies of the best candidate — equal scores leave in index order;
  * 3000 copies of the best candidate: S > K₀, the survivor pass runs;
  * NaN candidates (kept, first) on the reuse route;
  * N = 1300 under forced levels, M = 5003: the reuse switch and the first level's tail switch (fp64 / fp32) through all four
    combinations;
  * LogEI on a nearly noise-free model under an exact bound, candidates ON early training points: their stored bounds are −Inf — kept
    (the guard is NaN) but last by bound, so not among the threshold pass's candidates: the call runs the survivor pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

import ctypes as C

from tests.test_gpu_parity import make_model
from tests.test_gpu_kgen_tail32 import K, K0, NEVER, NOISE, SF2, _acq, _bits, _bounds, _force, _levels, _lib, _path_off, _tail32


def _reuse(mode):
    abo._lib.check(_lib().abo_test_prune_reuse(mode))


def _moduli(n):
    abo._lib.check(_lib().abo_test_prune_bound_moduli(n))


def _reused(model):
    out = C.c_int32(-1)
    abo._lib.check(_lib().abo_test_prune_reused(model._require(), C.byref(out)))
    return out.value


@pytest.fixture(autouse=True)
def _defaults():
    def reset():
        _force(0, 0)
        _levels(0, -1)
        _tail32(-1)
        _reuse(-1)
        _moduli(0)
    reset()
    yield
    reset()


@pytest.fixture(scope="module")
def n3072():
    X, y = synth.standardized_problem(3072, 8, 0.03)
    Z = synth.points(2, 20000, 8)
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, NOISE, contraction="int8"), X, y)
    return X, y, Z, model


def _call(acq, model, Z, reuse, force=(0, 0), levels=(0, -1)):
    _force(*force)
    _levels(*levels)
    _reuse(reuse)
    _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    return tv, ti, model.prune_stats(), model.prune_levels(), _reused(model)


def _same(a, b):
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))


@pytest.mark.parametrize("name", ["ei", "ucb"])
def test_threshold_scores_are_reused_below_k0(n3072, name):
    X, y, Z, model = n3072
    acq = _acq(name, y)
    off = _path_off(acq, model, Z)
    assert _reused(model) == 0
    tv, ti, st, lv, used = _call(acq, model, Z, 1)
    tv0, ti0, st0, lv0, used0 = _call(acq, model, Z, 0)
    print(f"{name}: reuse on {st} {lv} reused = {used}; off {st0} reused = {used0}")
    assert used == 1 and used0 == 0
    assert st["pruned"] == 1 and st0["pruned"] == 1 and K <= st["survivors"] <= K0
    assert st["survivors"] == st0["survivors"] and lv["level2_rows"] == 0
    _same((tv, ti), (tv0, ti0))
    _same((tv, ti), off)


def test_ties_leave_in_index_order(n3072):
    X, y, Z, model = n3072
    acq = _acq("ucb", y)
    _, best = _path_off(acq, model, Z)
    Zt = Z.copy()
    where = np.arange(137, 137 + 50 * 331, 331)
    Zt[where] = Z[best[0]]
    off = _path_off(acq, model, Zt)
    tv, ti, st, lv, used = _call(acq, model, Zt, 1)
    print(st, lv, used)
    assert used == 1 and st["pruned"] == 1
    _same((tv, ti), off)
    tied = np.flatnonzero(_bits(tv) == _bits(tv)[0])
    assert len(tied) >= 51 and np.all(np.diff(ti[tied]) > 0)          # equal scores: ascending indices


def test_more_survivors_than_k0_run_the_survivor_pass(n3072):
    X, y, Z, model = n3072
    acq = _acq("ucb", y)
    _, best = _path_off(acq, model, Z)
    Zt = Z.copy()
    Zt[np.arange(5, 5 + 3000 * 6, 6)] = Z[best[0]]
    off = _path_off(acq, model, Zt)
    tv, ti, st, lv, used = _call(acq, model, Zt, 1, levels=(0, NEVER))
    print(st, lv, used)
    assert st["survivors"] >= 3000 and used == 0 and st["pruned"] == 1 and lv["level2_rows"] == 0
    _same((tv, ti), off)


def test_nan_candidates_on_the_reuse_route(n3072):
    X, y, Z, model = n3072
    acq = _acq("ucb", y)
    Zt = Z.copy()
    Zt[30, 2] = np.nan
    Zt[4031, 5] = np.inf
    Zt[19999, 0] = -np.inf
    off = _path_off(acq, model, Zt)
    tv, ti, st, lv, used = _call(acq, model, Zt, 1)
    print(st, lv, used)
    assert used == 1 and st["pruned"] == 1
    assert list(ti[:3]) == [30, 4031, 19999] and np.isnan(tv[:3]).all() and not np.isnan(tv[3:]).any()
    _same((tv, ti), off)


def test_both_switches_through_all_combinations():
    N, d, M = 1300, 8, 5003
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, NOISE, contraction="int8"), X, y)
    acq = _acq("ei", y)
    off = _path_off(acq, model, Z)
    seen = []
    for tail in (0, 1):
        for reuse in (0, 1):
            _tail32(tail)
            tv, ti, st, lv, used = _call(acq, model, Z, reuse, force=(2, 0), levels=(1, -1))
            print(f"fp32 tail {tail}, reuse {reuse}: {st} {lv} reused = {used}")
            assert st["pruned"] == 1 and lv["level1_rows"] == 256
            assert used == (1 if reuse and lv["level2_rows"] == 0 and st["survivors"] <= K0 else 0)
            _same((tv, ti), off)
            seen.append(used)
    assert any(seen)


def test_minus_infinity_bounds_run_the_survivor_pass():
    N, d, M, noise = 1300, 8, 5003, 1e-13
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d).copy()
    early = [i for i in range(16) if y[i] > np.min(y) + 0.5][:6]      # among the bound's 256 rows, none of them the best point
    where = 100 + 37 * np.arange(len(early))
    Z[where] = X[early]
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, noise, contraction="int8"), X, y)
    acq = _acq("logei", y)
    off = _path_off(acq, model, Z)
    _moduli(14)                                                       # the exact bound: its variance at a training point is the noise
    tv, ti, st, lv, used = _call(acq, model, Z, 1)
    ub = _bounds(model, M)
    print(f"{st} {lv} reused = {used}; bounds at the copies {ub[where]}")
    _same((tv, ti), off)
    assert len(early) >= 3 and np.all(np.isneginf(ub[where]))         # the case is there …
    assert st["pruned"] == 1 and K <= st["survivors"] <= K0           # … on a call whose survivor count alone would allow the reuse
    assert used == 0
    tv0, ti0, st0, lv0, used0 = _call(acq, model, Z, 0)
    assert st0["survivors"] == st["survivors"] and used0 == 0
    _same((tv0, ti0), off)
    # without such candidates the same model and score reuse
    _, _, st1, _, used1 = _call(acq, model, synth.points(2, M, d), 1)
    print(f"no copies: {st1} reused = {used1}")
    assert used1 == (1 if st1["pruned"] == 1 and st1["survivors"] <= K0 else 0)
