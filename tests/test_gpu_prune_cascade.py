"""Two bound levels of the pruned top-k selection (csrc/acq.hip: prune_plan, prune_select): a first bound pass over
N/32 rows of L⁻¹ on all candidates sets the threshold τ, the N/8 pass runs on its survivors only (when more than 4·K₀ are left, or
when abo_test_prune_levels says so), the stored bounds become min(level 1, level 2) and the list is compacted again against the same τ.

Every case asks for EXACT equality of the k values and indices with the same call with the path off (abo_test_prune_force(0, 2)).
Shapes: N = 3072 is the smallest size at which the rule gives a first level (256 of 512 bound rows); N = 1536 takes one under forced
row blocks (2, first level 1).  d = 8 Matérn-5/2 and d = 3 SE (coordinates padded to 4), M = 20 000, k = 100, int8 engine.

Survivor counts expected from the CPU oracle (oracle/gp_oracle.py; candidates whose score at (μ, σ²_R) reaches the 100th exact score,
synth.standardized_problem(N, d, 0.03), synth.points(2, 20000, d); LogEI is a monotone function of EI, so its counts are EI's):
    N = 3072, Matérn-5/2 d = 8:   EI  809 at R = 256, 421 at R = 512;   UCB(2)  241, 176
    N = 1536, Matérn-5/2 d = 8:   EI  321 at R = 256, 204 at R = 512;   UCB(2)  219, 163
    N = 1536, SE ell 0.5 d = 3:   EI  358 at R = 256, 176 at R = 512;   UCB(2)  112, 110
all far below M/2 = 10 000 (the library's own counts are a little larger: its bound is taken at μ̃ − ε and on 8 moduli with a guard)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

from tests.test_gpu_parity import make_model

XI, BETA, K, M, K0 = 0.01, 2.0, 100, 20000, 1024
PRUNE_REL, PRUNE_ABS, PRUNE_ABS_LOGEI = 2.0 ** -30, 2.0 ** -1022, 2.0 ** -30          # csrc/abo_kernels.h
NEVER = 1 << 40                                                                       # level2_min no survivor count exceeds


def _force(rblocks, mode):
    abo._lib.check(abo._lib.lib().abo_test_prune_force(rblocks, mode))


def _levels(pre_rblocks, level2_min):
    abo._lib.check(abo._lib.lib().abo_test_prune_levels(pre_rblocks, level2_min))


@pytest.fixture(autouse=True)
def _defaults():
    _force(0, 0)
    _levels(0, -1)
    yield
    _force(0, 0)
    _levels(0, -1)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _acq(name, y):
    best = float(np.min(y))
    return {"ei": abo.ExpectedImprovement(XI, best), "logei": abo.LogExpectedImprovement(XI, best),
            "ucb": abo.UpperConfidenceBound(BETA)}[name]


def _bounds(model, m):
    ub = np.empty(m)
    abo._lib.check(abo._lib.lib().abo_test_prune_bounds(model._require(), ub.ctypes.data, m))
    return ub


def _kept(ub, tau, name):
    """prune_keep (csrc/misc.hip): a NaN on either side keeps the candidate"""
    with np.errstate(invalid="ignore"):
        return ~(ub + np.abs(ub) * PRUNE_REL + (PRUNE_ABS_LOGEI if name == "logei" else PRUNE_ABS) < tau)


def _call(acq, model, Z, k=K):
    _, tv, ti = abo.evaluate(acq, model, Z, k=k, return_scores=False)
    return tv, ti, model.prune_stats(), model.prune_levels()


def _full_path(acq, model, Z, force_rblocks, k=K):
    """the call with the path off, and the full pass's scores of all candidates"""
    _force(0, 2)
    _, tv0, ti0 = abo.evaluate(acq, model, Z, k=k, return_scores=False)
    assert model.prune_stats()["bound_rows"] == 0 and model.prune_levels()["level1_rows"] == 0
    _force(force_rblocks, 0)
    s, _, _ = abo.evaluate(acq, model, Z, k=0)
    return tv0, ti0, s


def _same(tv, ti, tv0, ti0):
    np.testing.assert_array_equal(ti, ti0)
    np.testing.assert_array_equal(_bits(tv), _bits(tv0))


def _level2_forced(name, y, Z, model, force_rblocks, pre_rblocks, rows1, rows2):
    """level 2 forced: selection = path off; S₁ and S₂ are the counts of guarded bounds reaching τ, the stored bounds dominate the
    exact scores; returns (statistics, levels)"""
    m = Z.shape[0]
    acq = _acq(name, y)
    tv0, ti0, s = _full_path(acq, model, Z, force_rblocks)
    # level 1 alone (level 2 never runs): its bounds, and from them τ as the library takes it — the k-th best exact score of the K₀
    # best by bound, NaN first and ties to the lowest index as everywhere
    _levels(pre_rblocks, NEVER)
    tv, ti, st, lv = _call(acq, model, Z)
    _same(tv, ti, tv0, ti0)
    assert lv["level1_rows"] == rows1 and lv["level2_rows"] == 0 and lv["level2_survivors"] == 0
    ub1 = _bounds(model, m)
    _, first = O.top_k(ub1, K0)
    tau = O.top_k(s[first], K)[0][K - 1]
    assert np.isfinite(tau)
    s1 = int(np.sum(_kept(ub1, tau, name)))
    assert lv["level1_survivors"] == s1 == st["survivors"]
    # both levels
    _levels(pre_rblocks, 0)
    tv, ti, st, lv = _call(acq, model, Z)
    print(f"{name} N-rows {rows1}/{rows2}: {st} {lv}")
    _same(tv, ti, tv0, ti0)
    assert st["pruned"] == 1 and st["fallback"] == 0 and st["bound_rows"] == rows1 and st["k0"] == K0
    assert lv["level1_rows"] == rows1 and lv["level2_rows"] == rows2 and lv["level1_survivors"] == s1
    s2 = lv["level2_survivors"]
    assert K <= s2 <= s1 and st["survivors"] == s2
    ub = _bounds(model, m)
    assert s2 == int(np.sum(_kept(ub, tau, name)))
    nan = np.isnan(ub)
    assert np.array_equal(nan, np.isnan(ub1)) and np.all(ub[~nan] <= ub1[~nan])
    keep1 = _kept(ub1, tau, name)
    assert np.array_equal(_bits(ub[~keep1]), _bits(ub1[~keep1]))               # level 2 never looked at what level 1 removed
    fin = ~nan & ~np.isnan(s)
    assert np.all(ub[fin] >= s[fin])                                          # NaN on either side: kept, nothing to compare
    assert np.all(np.isnan(s[nan]))                                           # a NaN bound belongs to a candidate whose score is NaN
    return st, lv


@pytest.fixture(scope="module")
def n3072():
    X, y = synth.standardized_problem(3072, 8, 0.03)
    return y, synth.points(2, M, 8), abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8"), X, y)


@pytest.fixture(scope="module")
def n1536_matern8():
    X, y = synth.standardized_problem(1536, 8, 0.03)
    return y, synth.points(2, M, 8), abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8"), X, y)


@pytest.fixture(scope="module")
def n1536_se3():
    X, y = synth.standardized_problem(1536, 3, 0.03)
    return y, synth.points(2, M, 3), abo.update(make_model(O.SE, 0.5, 1.5, 1e-3, contraction="int8"), X, y)


@pytest.mark.parametrize("name", ["ei", "logei", "ucb"])
def test_rule_path_has_a_first_level_of_256_rows(n3072, name):
    y, Z, model = n3072
    acq = _acq(name, y)
    tv0, ti0, _ = _full_path(acq, model, Z, 0)
    tv, ti, st, lv = _call(acq, model, Z)
    print(f"{name}: {st} {lv}")
    _same(tv, ti, tv0, ti0)
    assert lv["level1_rows"] == 256 and st["bound_rows"] == 256 and st["pruned"] == 1 and st["fallback"] == 0
    assert K <= st["survivors"] < M // 2
    # 4·K₀ = 4096 survivors are not reached here: the second level is skipped and the first level's list is the survivor list
    assert lv["level1_survivors"] <= 4 * K0 and lv["level2_rows"] == 0 and st["survivors"] == lv["level1_survivors"]


@pytest.mark.parametrize("name", ["ei", "logei", "ucb"])
def test_level_two_forced(n3072, name):
    y, Z, model = n3072
    st, lv = _level2_forced(name, y, Z, model, 0, 0, 256, 512)
    assert st["survivors"] < M // 2


@pytest.mark.parametrize("name", ["ei", "logei", "ucb"])
@pytest.mark.parametrize("which", ["n1536_matern8", "n1536_se3"])
def test_level_two_forced_under_forced_row_blocks(request, which, name):
    """N = 1536 with two row blocks forced and a first level of one: δ's row index crosses 128 and 256 in the second level"""
    y, Z, model = request.getfixturevalue(which)
    st, lv = _level2_forced(name, y, Z, model, 2, 1, 256, 512)
    assert st["survivors"] < M // 2


def test_ragged_and_degenerate_lists():
    """M = 20 003 in chunks of 512 (so both levels run more than one chunk), 13 copies of the candidate ranked 95th straddling the first
    chunk boundary (k = 100 cuts the tie), three candidates with a NaN or Inf coordinate"""
    m = 20003
    X, y = synth.standardized_problem(3072, 8, 0.03)
    model = abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8", chunk=512), X, y)
    Z = synth.points(2, m, 8).copy()
    acq = _acq("ei", y)
    s, _, _ = abo.evaluate(acq, model, Z, k=0)
    j95 = int(O.top_k(s, K)[1][94])
    Z[506:518] = Z[j95]
    bad = [300, 9000, m - 1]
    assert j95 not in bad and not 506 <= j95 < 518
    Z[300, 2] = np.nan
    Z[9000, 5] = np.inf
    Z[m - 1, 0] = -np.inf
    tv0, ti0, s = _full_path(acq, model, Z, 0)
    assert list(ti0[:3]) == bad and np.isnan(tv0[:3]).all() and not np.isnan(tv0[3:]).any()
    assert np.sum(s == s[j95]) == 13 > np.sum(tv0 == s[j95]) >= 1             # more candidates hold the tied score than were selected
    _levels(0, 0)
    tv, ti, st, lv = _call(acq, model, Z)
    print(st, lv)
    _same(tv, ti, tv0, ti0)
    assert st["pruned"] == 1 and lv["level1_rows"] == 256 and lv["level2_rows"] == 512
    assert K <= lv["level2_survivors"] <= lv["level1_survivors"] < m // 2
    ub = _bounds(model, m)
    assert np.isnan(ub[bad]).all() and np.sum(np.isnan(ub)) == 3              # kept by both levels
    assert len(set(_bits(ub[506:518]))) == 1 and ub[506] == ub[j95]           # one candidate, one bound, wherever it stands in a list
    fin = ~np.isnan(ub)
    assert np.all(ub[fin] >= s[fin])


def test_threshold_of_minus_infinity_runs_level_two_over_all_candidates(n3072):
    y, Z, model = n3072
    acq = _acq("ei", y)
    tv0, ti0, s = _full_path(acq, model, Z, 0)
    _force(0, 1)
    tv, ti, st, lv = _call(acq, model, Z)
    print(st, lv)
    _same(tv, ti, tv0, ti0)
    assert (lv["level1_rows"], lv["level1_survivors"], lv["level2_rows"], lv["level2_survivors"]) == (256, M, 512, M)
    assert st["fallback"] == 1 and st["pruned"] == 0 and st["survivors"] == M and st["bound_rows"] == 256
    ub = _bounds(model, M)
    assert np.all(ub >= s)
    # the timings count every pass that ran: two bound passes, the threshold pass, the full pass
    assert model.timings()["var_gemm_flop"] == 256.0 ** 2 * M + 512.0 ** 2 * M + 3072.0 ** 2 * (K0 + M)


def test_without_a_first_level_the_call_is_the_single_level_one(n3072):
    y, Z, model = n3072
    acq = _acq("ei", y)
    tv0, ti0, s = _full_path(acq, model, Z, 0)
    _levels(-1, -1)
    tv, ti, st, lv = _call(acq, model, Z)
    print(st, lv)
    _same(tv, ti, tv0, ti0)
    assert lv == {"level1_rows": 0, "level1_survivors": 0, "level2_rows": 0, "level2_survivors": 0, "level1_ms": 0.0, "level2_ms": 0.0}
    assert st["bound_rows"] == 256 * 2 and st["pruned"] == 1 and K <= st["survivors"] < M // 2
    ub = _bounds(model, M)
    assert np.all(ub >= s)


def test_a_forced_first_level_not_below_the_bound_pass_is_refused(n3072):
    y, Z, model = n3072
    _levels(2, -1)                                                            # the bound pass has 2 row blocks at N = 3072
    with pytest.raises(ValueError, match="not below"):
        abo.evaluate(_acq("ei", y), model, Z, k=K, return_scores=False)


def test_two_handles_used_alternately(n3072, n1536_matern8):
    """both with a first level of 256 and a second of 512 rows (forced row blocks 2 = the rule's at N = 3072): planes, row scales and
    bounds of one handle's levels must not reach the other's"""
    ya, Za, a = n3072
    yb, Zb, b = n1536_matern8
    Zb = Zb[:15001]
    acq_a, acq_b = _acq("ei", ya), _acq("ei", yb)
    ref_a, ref_b = _full_path(acq_a, a, Za, 2), _full_path(acq_b, b, Zb, 2)
    _levels(1, 0)
    seen = []
    for _ in range(2):
        for acq, model, Z, ref in ((acq_a, a, Za, ref_a), (acq_b, b, Zb, ref_b)):
            tv, ti, st, lv = _call(acq, model, Z)
            _same(tv, ti, ref[0], ref[1])
            assert st["pruned"] == 1 and lv["level1_rows"] == 256 and lv["level2_rows"] == 512
            ub = _bounds(model, Z.shape[0])
            assert np.all(ub >= ref[2])
            seen.append((lv["level1_survivors"], lv["level2_survivors"], _bits(ub).copy()))
    for i in (0, 1):                                                          # the second round repeats the first bit for bit
        assert seen[i][:2] == seen[i + 2][:2] and np.array_equal(seen[i][2], seen[i + 2][2])
