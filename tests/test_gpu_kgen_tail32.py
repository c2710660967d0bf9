"""The fp32 tail of the FIRST bound level of the pruned top-k selection (csrc/kgen_tail32.hip, csrc/abo_kappa.h: kappa_tail32;
DESIGN.md §3b-1) on the device.  int8 engine, k = 100; every selection is asked to equal, bit for bit, the same call with the path off
(abo_test_prune_force(0, 2)).

  * kappa_tail32 against 60-digit mpmath for every family: within TAIL32_ETA_EVAL of κ, clamp and underflow end included;
  * N = 3072 (the smallest size with a rule-given first level), M = 20 000: |μ̃ − μ| ≤ ε for every candidate (μ from the library's full
    pass, and from the oracle on 2000 rows), ε no larger than the formula of kgen_tail32.hip evaluated here from α and the constants,
    EI / LogEI / UCB(2) selections unchanged, level-1 survivors ≤ 4·K₀;
  * N = 1300 and 1536 under forced row blocks 2 with a forced first level of 1: every family × every padded dimension (the 24
    instantiations), M = 5003 (no multiple of 16);
  * adversarial candidates, and a model after a bordered append (N = 1301 in padded storage);
  * the switch (ABO_PRUNE_TAIL32=0 through its hook): the stored level-1 bounds are the parent commit's, by hash."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

from tests.test_gpu_parity import make_model
from tests.test_kgen_tail32_cpu import C, U, V1

SF2, NOISE, XI, BETA, K, K0 = 1.0, 1e-3, 0.01, 2.0, 100, 1024
NEVER = 1 << 40
# sha256 of the level-1 bounds (abo_test_prune_bounds, 20 000 doubles) of the EI call of the n3072 fixture below, as computed by a build
# of the parent commit (fp64 tail in the first level) on an MI355X
PARENT_UB_SHA256 = "07b078c0a022f9b0fe32ed8ef3ef4b7f7d8fad33db780011af8fa21970c693d5"
# level-1 survivors of the same call with the fp64 tail (tests/test_gpu_prune_cascade.py's header)
FP64_S1_N3072_EI = 809


def _lib():
    return abo._lib.lib()


def _force(rblocks, mode):
    abo._lib.check(_lib().abo_test_prune_force(rblocks, mode))


def _levels(pre_rblocks, level2_min):
    abo._lib.check(_lib().abo_test_prune_levels(pre_rblocks, level2_min))


def _tail32(mode):
    abo._lib.check(_lib().abo_test_prune_tail32(mode))


@pytest.fixture(autouse=True)
def _defaults():
    def reset():
        _force(0, 0)
        _levels(0, -1)
        _tail32(-1)
    reset()
    yield
    reset()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _acq(name, y):
    best = float(np.min(y))
    return {"ei": abo.ExpectedImprovement(XI, best), "logei": abo.LogExpectedImprovement(XI, best), "ucb": abo.UpperConfidenceBound(BETA)}[name]


def _alpha(model, N):
    a = np.empty(N)
    abo._lib.check(_lib().abo_get_factor(model._require(), None, a.ctypes.data, None))
    return a


def _mean_eps(model, M):
    mu_t, eps = np.empty(M), np.empty(M)
    abo._lib.check(_lib().abo_test_prune_mean(model._require(), mu_t.ctypes.data, eps.ctypes.data, M))
    return mu_t, eps


def _bounds(model, M):
    ub = np.empty(M)
    abo._lib.check(_lib().abo_test_prune_bounds(model._require(), ub.ctypes.data, M))
    return ub


def _path_off(acq, model, Z):
    _force(0, 2)
    _, tv0, ti0 = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    assert model.prune_stats()["bound_rows"] == 0
    return tv0, ti0


def _first_level_call(acq, model, Z, force_rblocks, pre_rblocks, level2_min=-1):
    """the call with a first level of 256 rows, after the same call with the path off: same bits; → statistics, levels, (μ̃, ε) of level 1"""
    tv0, ti0 = _path_off(acq, model, Z)
    _force(force_rblocks, 0)
    _levels(pre_rblocks, level2_min)
    _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    st, lv = model.prune_stats(), model.prune_levels()
    np.testing.assert_array_equal(ti, ti0)
    np.testing.assert_array_equal(_bits(tv), _bits(tv0))
    assert st["bound_rows"] == 256 and lv["level1_rows"] == 256
    mu_t, eps = _mean_eps(model, Z.shape[0])
    return tv, ti, st, lv, mu_t, eps


def _eps_formula(X, Z, ell, alpha, dp, rows, Np, sf2=SF2, mean_c=0.0):
    """ε of kgen_tail32.hip from the scaled inputs, α and the constants of abo_kappa.h"""
    xs, zs = X / ell, Z / ell
    w = np.max(np.sum(xs[rows:] ** 2, axis=1)) + np.sum(zs ** 2, axis=1)
    eta = C["TAIL32_ETA_EVAL"] + C["TAIL32_REL_R"] * (0.5 * dp + 1.0) * V1 + C["TAIL32_LIP_R"] * (V1 * np.sqrt(2.0 * w) + C["TAIL32_R_ABS"])
    a_tail, a_all = np.sum(np.abs(alpha[rows:])), np.sum(np.abs(alpha))
    return 1.0001 * sf2 * ((eta + (dp + 14) * U) * a_tail + (2.0 * Np + 64.0) * U * a_all) + 8.0 * U * abs(mean_c)


@pytest.mark.parametrize("family", [O.SE, O.MATERN52, O.MATERN72, O.MATERN32])
def test_kappa_tail32_within_its_stated_distance(family):
    import mpmath as mp
    import torch
    mp.mp.dps = 60
    rng = np.random.default_rng(320 + family)
    edge = []
    for s in (0.5, 3.0 ** 0.5, 5.0 ** 0.5, 7.0 ** 0.5):              # the scaled exponent around −126 (denormal result) and −150 (clamp)
        for t in (-125.0, -126.5, -140.0, -149.5, -150.5, -200.0):
            a = -t / 1.44269504088896340736
            edge += [(a / s) ** 2, 2.0 * a]
    d2 = np.concatenate([[0.0, 1e-45, 1e-40, 2.0 ** -126, 1e-30, 1e-13, 1e-12, 1e-10, 1e-6, 0.5, 1.0, 2.0, 100.0, 1e3, 1e5, 2e5, 1e6, 1e9, 1e12, 2.0 ** 41],
                         edge, 10.0 ** rng.uniform(-8, 3, 1500), rng.uniform(0, 50, 1500)]).astype(np.float32).astype(np.float64)
    x = torch.from_numpy(d2).cuda()
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    abo._lib.check(_lib().abo_test_kappa_tail32(0, family, x.data_ptr(), out.data_ptr(), x.numel()))
    got = out.cpu().numpy()

    def exact(v):
        v = mp.mpf(float(v))
        if family == O.SE:
            return mp.exp(-v / 2)
        r = mp.sqrt(v)
        if family == O.MATERN52:
            return (1 + mp.sqrt(5) * r + 5 * v / 3) * mp.exp(-mp.sqrt(5) * r)
        if family == O.MATERN72:
            return (1 + mp.sqrt(7) * r + mp.mpf(14) / 5 * v + 7 * mp.sqrt(7) / 15 * v * r) * mp.exp(-mp.sqrt(7) * r)
        return (1 + mp.sqrt(3) * r) * mp.exp(-mp.sqrt(3) * r)

    ref = np.array([float(exact(v)) for v in d2])
    err = np.abs(got - ref)
    print(f"family {family}: max |kappa_tail32 - kappa| = {err.max():.3e} = {err.max() * 2.0 ** 24:.2f} v at r2 = {d2[np.argmax(err)]:.6g} "
          f"(stated: {C['TAIL32_ETA_EVAL']:.3e})")
    assert np.all(np.isfinite(got))                                   # (NaN: the halves of the packed pair disagreed)
    assert np.all(err <= C["TAIL32_ETA_EVAL"])
    assert got[0] == 1.0 and np.all(got[d2 >= 2.0e4] == 0.0)


@pytest.fixture(scope="module")
def n3072():
    X, y = synth.standardized_problem(3072, 8, 0.03)
    Z = synth.points(2, 20000, 8)
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, NOISE, contraction="int8"), X, y)
    mu, _ = abo.mean_and_var(model, Z)
    mu_o, _ = O.predict(O.fit(O.MATERN52, 1.0, SF2, NOISE, 0.0, X, y), Z[:2000])
    return X, y, Z, model, mu, mu_o


def test_guard_at_the_smallest_rule_given_first_level(n3072):
    X, y, Z, model, mu, mu_o = n3072
    M = Z.shape[0]
    tv, ti, st, lv, mu_t, eps = _first_level_call(_acq("ei", y), model, Z, 0, 0)
    err, err_o = np.abs(mu_t - mu), np.abs(mu_t[:2000] - mu_o)
    alpha = _alpha(model, 3072)
    want = _eps_formula(X, Z, 1.0, alpha, 8, 256, 3072)
    print(f"N = 3072: {st} {lv}")
    print(f"  |alpha_tail|_1 = {np.sum(np.abs(alpha[256:])):.4e}; eps median {np.median(eps):.4e}, max {eps.max():.4e}; max|mu~ - mu| = {err.max():.3e} "
          f"(max err/eps = {np.max(err / eps):.3e}); against the oracle on 2000 rows {err_o.max():.3e}")
    assert np.all(np.isfinite(mu_t)) and np.all(eps > 0.0)
    assert np.all(err <= eps) and np.all(err_o <= eps[:2000])
    assert np.all(eps <= want * (1.0 + 1e-12))
    # survivor growth: the cascade test's own condition (level 2 not needed) holds with the fp32 tail
    s32 = lv["level1_survivors"]
    _tail32(0)
    _, _, st64, lv64, mu64, eps64 = _first_level_call(_acq("ei", y), model, Z, 0, 0)
    print(f"  level-1 survivors: {s32} with the fp32 tail, {lv64['level1_survivors']} with the fp64 tail ({FP64_S1_N3072_EI} recorded); "
          f"fp64 eps max {eps64.max():.3e}")
    assert s32 <= 4 * K0 and lv["level2_rows"] == 0 and st["survivors"] == s32


@pytest.mark.parametrize("name", ["logei", "ucb"])
def test_other_monotone_scores_at_the_rule_given_first_level(n3072, name):
    X, y, Z, model, mu, mu_o = n3072
    tv, ti, st, lv, mu_t, eps = _first_level_call(_acq(name, y), model, Z, 0, 0)
    print(f"{name}: {st} {lv}")
    assert st["pruned"] == 1 and lv["level1_survivors"] <= 4 * K0
    assert np.all(np.abs(mu_t - mu) <= eps)


def test_second_level_keeps_the_fp64_tail(n3072):
    """level 2 forced: its ε (the buffers of its own are not exposed) shows in the bounds — where level 2 looked, the stored bound is
    the smaller of the two, and the selection is unchanged"""
    X, y, Z, model, mu, mu_o = n3072
    tv, ti, st, lv, mu_t, eps = _first_level_call(_acq("ei", y), model, Z, 0, 0, level2_min=0)
    print(st, lv)
    assert lv["level2_rows"] == 512 and K <= lv["level2_survivors"] <= lv["level1_survivors"]
    ub = _bounds(model, Z.shape[0])
    s, _, _ = abo.evaluate(_acq("ei", y), model, Z, k=0)
    assert np.all(ub >= s)


def test_single_level_calls_keep_the_fp64_tail(n3072):
    X, y, Z, model, mu, mu_o = n3072
    acq = _acq("ei", y)
    tv0, ti0 = _path_off(acq, model, Z)
    _force(0, 0)
    _levels(-1, -1)
    _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    np.testing.assert_array_equal(ti, ti0)
    np.testing.assert_array_equal(_bits(tv), _bits(tv0))
    assert model.prune_stats()["bound_rows"] == 512 and model.prune_levels()["level1_rows"] == 0
    mu_t, eps = _mean_eps(model, Z.shape[0])
    a_tail = float(np.sum(np.abs(_alpha(model, 3072)[512:])))
    assert np.all(eps <= 2.0 ** -30 * SF2 * a_tail)                   # tests/test_gpu_kgen_tail.py's cap: far below any fp32 guard


def test_switch_gives_the_parent_commits_level_one_bounds(n3072):
    X, y, Z, model, mu, mu_o = n3072
    _tail32(0)
    _first_level_call(_acq("ei", y), model, Z, 0, 0, level2_min=NEVER)
    ub = _bounds(model, Z.shape[0])
    got = hashlib.sha256(np.ascontiguousarray(ub).tobytes()).hexdigest()
    print(f"sha256 of the level-1 bounds with the switch off: {got}")
    assert got == PARENT_UB_SHA256
    _tail32(1)
    _first_level_call(_acq("ei", y), model, Z, 0, 0, level2_min=NEVER)
    ub32 = _bounds(model, Z.shape[0])
    assert np.any(_bits(ub32) != _bits(ub))                           # the switch does switch


DIMS = [(1, 0.2), (2, 0.3), (3, 0.5), (5, 0.8), (8, 1.0), (16, 1.5), (32, 2.0)]


@pytest.mark.parametrize("family", [O.SE, O.MATERN52, O.MATERN72, O.MATERN32])
@pytest.mark.parametrize("d,ell", DIMS)
def test_ragged_shapes_every_instantiation(family, d, ell):
    N = 1300 if (d + family) % 2 else 1536
    M = 5003
    dp = 1 if d == 1 else 2 if d == 2 else 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(family, ell, SF2, NOISE, contraction="int8"), X, y)
    tv, ti, st, lv, mu_t, eps = _first_level_call(_acq("ei", y), model, Z, 2, 1)
    mu, _ = abo.mean_and_var(model, Z)
    err = np.abs(mu_t - mu)
    want = _eps_formula(X, Z, ell, _alpha(model, N), dp, 256, 1536)
    print(f"family {family} d={d} N={N}: {st} {lv}; eps max {eps.max():.3e}, max|mu~ - mu| = {err.max():.3e}, max err/eps = {np.max(err / eps):.3e}")
    assert np.all(np.isfinite(mu_t)) and np.all(err <= eps)
    assert np.all(eps <= want * (1.0 + 1e-9))                         # (the library scales by a rounded 1/ℓ)


def _adversarial(N):
    d, M = 8, 5003
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d).copy()
    Z[10] = X[300]                                                    # on a training point of the tail (index ≥ 256)
    Z[11] = X[700] + 1e-12                                            # … and next to one: the inputs' rounding is all of the distance
    Z[12] = X[N - 1]
    Z[20:24] += 1000.0                                                # exponent beyond the clamp, a large w
    Z[30, 2] = np.nan
    Z[31, 5] = np.inf
    Z[32, 0] = -np.inf
    Z[33, 1] = 1e25                                                   # finite, its square beyond fp32 and TAIL_W_MAX: out of range, kept
    return X, y, Z


def test_adversarial_candidates():
    N = 1300
    X, y, Z = _adversarial(N)
    M = Z.shape[0]
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, NOISE, contraction="int8"), X, y)
    tv, ti, st, lv, mu_t, eps = _first_level_call(_acq("ei", y), model, Z, 2, 1)
    print(st, lv)
    bad = np.array([30, 31, 32])
    assert list(ti[:3]) == [30, 31, 32] and np.isnan(tv[:3]).all() and not np.isnan(tv[3:]).any()
    assert np.isnan(mu_t[bad]).all() and np.isnan(mu_t[33])           # non-finite and out-of-range candidates: μ̃ = NaN, kept
    ub = _bounds(model, M)
    assert np.isnan(ub[bad]).all() and np.isnan(ub[33])
    ok = np.ones(M, bool)
    ok[[30, 31, 32, 33]] = False
    mu, _ = abo.mean_and_var(model, Z)
    assert np.all(np.isfinite(mu_t[ok])) and np.all(np.isfinite(eps[ok]))
    err = np.abs(mu_t - mu)
    for j in (10, 11, 12, 20, 23):
        print(f"  candidate {j}: mu~ - mu = {mu_t[j] - mu[j]:.3e}, eps = {eps[j]:.3e}")
    assert np.all(err[ok] <= eps[ok])
    box = ok.copy()
    box[20:24] = False
    assert np.all(eps[20:24] > eps[box].max())                        # the far candidates carry the larger, w-dependent ε
    s, _, _ = abo.evaluate(_acq("ei", y), model, Z, k=0)
    fin = ~np.isnan(ub) & ~np.isnan(s)
    assert np.all(ub[fin] >= s[fin])


def test_after_an_append_the_padding_is_not_read():
    from abstractbayesopt.jl_amd import incremental
    N, d, M = 1300, 8, 5003
    X, y = synth.standardized_problem(N + 1, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, NOISE, contraction="int8"), X[:N], y[:N])
    model = incremental.append(model, X[N], float(y[N]))
    tv, ti, st, lv, mu_t, eps = _first_level_call(_acq("ei", y), model, Z, 2, 1)
    print(st, lv)
    mu, _ = abo.mean_and_var(model, Z)
    err = np.abs(mu_t - mu)
    print(f"  max|mu~ - mu| = {err.max():.3e}, max err/eps = {np.max(err / eps):.3e}")
    assert np.all(err <= eps)
    # the fp64 tail on the same handle sums the same columns: were a padding row or a padding weight read by one of the two alone,
    # the two means would differ by more than the two guards allow
    _tail32(0)
    _, _, _, _, mu64, eps64 = _first_level_call(_acq("ei", y), model, Z, 2, 1)
    assert np.all(np.abs(mu_t - mu64) <= eps + eps64)
    mu_o, _ = O.predict(O.fit(O.MATERN52, 1.0, SF2, NOISE, 0.0, X, y), Z[:1000])
    assert np.all(np.abs(mu_t[:1000] - mu_o) <= eps[:1000] + 1e-6 * max(1.0, float(np.max(np.abs(mu_o)))))
