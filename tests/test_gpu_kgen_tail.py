"""The μ-only tail of the pruned selection's bound pass (csrc/kgen_tail.hip, csrc/abo_kappa.h: kappa_tail).

For the training columns past the bound pass's row blocks the mean is summed with shortened arithmetic (expanded squared distance, one
step on the rsq seed, a degree-10 exponential) and the pass scores at μ̃ − ε, ε a proven bound of |μ̃ − μ|.  Checked here, int8 engine,
EI, k = 100:
  * |μ̃_j − μ_j| ≤ ε_j for every candidate, μ from the library's full pass; both agree with the oracle's mean at the tolerance of
    tests/test_gpu_parity.py (max |Δμ| / max(1, max|μ|) ≤ 1e-6);
  * ε_j ≤ 2⁻³⁰·σ_f²·Σ_{k ≥ R}|α_k| for candidates in the unit box (the guard is not vacuous), α from abo_get_factor;
  * adversarial candidates (on a tail training point, 1e-12 from one, +1000 per coordinate, NaN, Inf): same bits as the path off,
    non-finite candidates have μ̃ = NaN and rank first;
  * the survivor count stays within 1 % of M of the parent commit's;
  * kappa_tail against 60-digit mpmath: within TAIL_ETA_EVAL = 2⁻⁴¹ of κ (the constant the guard is built on)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

from tests.test_gpu_parity import make_model

SF2, NOISE, XI, K = 1.0, 1e-3, 0.01, 100
R = 256                                                  # training columns of the bound pass at these sizes (one row block)
TAIL_ETA_EVAL, TAIL_LIP, TAIL_R2_MIN = 2.0 ** -41, 1.5, 2.0 ** -200     # csrc/abo_kappa.h
# survivors of the EI call of tests/test_gpu_acq_prune.py::test_typical_case_prunes_and_bounds_dominate (N = 1536, M = 20000) as
# printed on the parent commit, whose bound pass took μ from the full generator
PARENT_SURVIVORS_TYPICAL = 321


def _force(rblocks, mode):
    abo._lib.check(abo._lib.lib().abo_test_prune_force(rblocks, mode))


@pytest.fixture(autouse=True)
def _defaults():
    _force(0, 0)
    yield
    _force(0, 0)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _alpha(model, N):
    a = np.empty(N)
    abo._lib.check(abo._lib.lib().abo_get_factor(model._require(), None, a.ctypes.data, None))
    return a


def _pruned_call(model, y, Z):
    """EI top-100 with the path on — after asserting that the call with the path off returns the same bits — then the bound pass's
    (μ̃, ε) and the call's statistics"""
    acq = abo.ExpectedImprovement(XI, float(np.min(y)))
    _force(0, 2)
    _, tv0, ti0 = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    assert model.prune_stats()["bound_rows"] == 0
    _force(0, 0)
    _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    st = model.prune_stats()
    np.testing.assert_array_equal(ti, ti0)
    np.testing.assert_array_equal(_bits(tv), _bits(tv0))
    assert st["bound_rows"] == R
    M = Z.shape[0]
    mu_t, eps = np.empty(M), np.empty(M)
    abo._lib.check(abo._lib.lib().abo_test_prune_mean(model._require(), mu_t.ctypes.data, eps.ctypes.data, M))
    return tv, ti, st, mu_t, eps


def _check_case(family, d, ell, N, M, oracle_rows=2000):
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(family, ell, SF2, NOISE, contraction="int8"), X, y)
    tv, ti, st, mu_t, eps = _pruned_call(model, y, Z)
    mu, _ = abo.mean_and_var(model, Z)
    alpha = _alpha(model, N)
    a_tail = float(np.sum(np.abs(alpha[R:])))
    err = np.abs(mu_t - mu)
    print(f"family {family} d={d} N={N} M={M}: {st}")
    print(f"  max|mu~ - mu| = {err.max():.3e}, eps in [{eps.min():.3e}, {eps.max():.3e}], max err/eps = {np.max(err / eps):.3e}, "
          f"cap 2^-30*sf2*|alpha_tail|_1 = {2.0 ** -30 * SF2 * a_tail:.3e}, |alpha_tail|_1 = {a_tail:.3e}")
    assert np.all(np.isfinite(mu_t)) and np.all(eps > 0.0)
    assert np.all(err <= eps)
    assert np.all(eps <= 2.0 ** -30 * SF2 * a_tail)
    sl = slice(0, min(M, oracle_rows))
    mu_o, _ = O.predict(O.fit(family, ell, SF2, NOISE, 0.0, X, y), Z[sl])
    scale = max(1.0, float(np.max(np.abs(mu_o))))
    d_full, d_tail = np.max(np.abs(mu[sl] - mu_o)) / scale, np.max(np.abs(mu_t[sl] - mu_o)) / scale
    print(f"  against the oracle: full pass {d_full:.3e}, bound pass {d_tail:.3e}")
    assert d_full <= 1e-6 and d_tail <= 1e-6
    return st


def test_typical_shape_error_within_eps_and_survivor_growth():
    M = 20000
    st = _check_case(O.MATERN52, 8, 1.0, 1536, M)                     # R = 256: five of six row blocks run the shortened path
    print(f"survivors: {st['survivors']} with the shortened tail, {PARENT_SURVIVORS_TYPICAL} on the parent commit")
    assert st["pruned"] == 1
    assert st["survivors"] <= PARENT_SURVIVORS_TYPICAL + M // 100


@pytest.mark.parametrize("d,ell", [(1, 0.2), (3, 0.5), (8, 1.0), (16, 1.5)])
def test_ragged_shape_every_padded_dimension(d, ell):
    _check_case(O.MATERN52, d, ell, 1300, 5000)                       # dp = 1, 4 (padded), 8, 16; ragged last row block


@pytest.mark.parametrize("family", [O.SE, O.MATERN72, O.MATERN32])
def test_ragged_shape_every_family(family):
    _check_case(family, 8, 1.0, 1300, 5000)


def test_adversarial_candidates():
    N, d, M = 1300, 8, 5000
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d).copy()
    Z[10] = X[300]                                                    # on a training point of the tail (index ≥ R): cancellation, clamp
    Z[11] = X[700] + 1e-12                                            # … and next to one: sqrt near 0
    Z[12] = X[1299]
    Z[20:24] += 1000.0                                                # exp underflow, a large |z|² in the cancellation term
    Z[30, 2] = np.nan
    Z[31, 5] = np.inf
    Z[32, 0] = -np.inf
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, NOISE, contraction="int8"), X, y)
    tv, ti, st, mu_t, eps = _pruned_call(model, y, Z)
    print(st)
    bad = np.array([30, 31, 32])
    assert list(ti[:3]) == [30, 31, 32] and np.isnan(tv[:3]).all() and not np.isnan(tv[3:]).any()
    assert np.isnan(mu_t[bad]).all()
    ok = np.ones(M, bool)
    ok[bad] = False
    mu, _ = abo.mean_and_var(model, Z)
    assert np.isnan(mu[bad]).all() and np.all(np.isfinite(mu_t[ok])) and np.all(np.isfinite(eps[ok]))
    err = np.abs(mu_t - mu)
    for j in (10, 11, 12, 20, 23):
        print(f"  candidate {j}: mu~ - mu = {mu_t[j] - mu[j]:.3e}, eps = {eps[j]:.3e}")
    print(f"  max err/eps over the finite candidates = {np.max(err[ok] / eps[ok]):.3e}")
    assert np.all(err[ok] <= eps[ok])
    # the far candidates carry the larger, |z|²-dependent ε; the unit-box ones stay under the cap
    a_tail = float(np.sum(np.abs(_alpha(model, N)[R:])))
    box = ok.copy()
    box[20:24] = False
    assert np.all(eps[box] <= 2.0 ** -30 * SF2 * a_tail) and np.all(eps[20:24] > eps[box].max())


def test_after_an_append_the_padding_is_not_read():
    """A bordered append leaves N = 1301 points in storage padded to whole blocks: the tail must stop at the last training point
    whatever the padding rows of the scaled inputs and of alpha hold."""
    from abstractbayesopt.jl_amd import incremental
    N, d, M = 1300, 8, 5000
    X, y = synth.standardized_problem(N + 1, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(O.MATERN52, 1.0, SF2, NOISE, contraction="int8"), X[:N], y[:N])
    model = incremental.append(model, X[N], float(y[N]))
    tv, ti, st, mu_t, eps = _pruned_call(model, y, Z)
    print(st)
    mu, _ = abo.mean_and_var(model, Z)
    err = np.abs(mu_t - mu)
    print(f"  max|mu~ - mu| = {err.max():.3e}, max err/eps = {np.max(err / eps):.3e}")
    assert np.all(err <= eps)
    a_tail = float(np.sum(np.abs(_alpha(model, N + 1)[R:])))
    assert np.all(eps <= 2.0 ** -30 * SF2 * a_tail)
    mu_o, _ = O.predict(O.fit(O.MATERN52, 1.0, SF2, NOISE, 0.0, X, y), Z[:1000])
    assert np.max(np.abs(mu_t[:1000] - mu_o)) / max(1.0, float(np.max(np.abs(mu_o)))) <= 1e-6


@pytest.mark.parametrize("family", [O.SE, O.MATERN52, O.MATERN72, O.MATERN32])
def test_kappa_tail_within_its_stated_distance(family):
    import mpmath as mp
    import torch
    mp.mp.dps = 60
    rng = np.random.default_rng(100 + family)
    d2 = np.concatenate([[0.0, 1e-300, 1e-200, 1e-60, 1e-30, 1e-13, 1e-12, 1e-10, 1e-6, 0.5, 1.0, 2.0, 100.0, 1e3, 1e5, 2e5, 1e6, 1e9, 1e12],
                         10.0 ** rng.uniform(-8, 3, 1500), rng.uniform(0, 50, 1500)])
    x = torch.from_numpy(d2).cuda()
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    abo._lib.check(abo._lib.lib().abo_test_kappa_tail(0, family, x.data_ptr(), out.data_ptr(), x.numel()))
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
    print(f"family {family}: max |kappa_tail - kappa| = {err.max():.3e} at r2 = {d2[np.argmax(err)]:.6g} (stated: {TAIL_ETA_EVAL:.3e})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= TAIL_ETA_EVAL + TAIL_LIP * TAIL_R2_MIN)
