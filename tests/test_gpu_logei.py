"""GPU tests (-m gpu) of LogEI (ABO_ACQ_LOGEI = 5; csrc/abo_acq_dev.h: log_h): the device arithmetic against the mpmath
table tests/golden/logei_kat.npz, its consistency and common order with EI, the same bits through every entry point that takes a
kind, the analytic gradient, the refinement in the regime where EI's own refinement does not start, and the pruned top-k selection.

The CPU restatement of LogEI (tests/test_logei_cpu.py: logei_restated) on the oracle's posterior is the reference wherever a model is
involved.  Achieved errors of the device arithmetic are DATA in tests/golden/logei_bounds.json (measured on an MI355X by this file);
a figure is asserted at 100 × its recorded value and at the hard bar the test states."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import acquisition as A
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

from tests.test_gpu_parity import make_model
from tests.test_logei_cpu import PARTIAL_BAR, load_golden, logei_restated, partial_error, value_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EI, UCB, LOGEI = 0, 1, 5
VALUE_CEILING = 1e-12                  # |got − ref| ≤ 1e-12·max(1, |ref|): a condition on the branch layout, not a measurement
PRUNE_REL, PRUNE_ABS, PRUNE_ABS_LOGEI = 2.0 ** -30, 2.0 ** -1022, 2.0 ** -30          # csrc/abo_kernels.h

with open(os.path.join(ROOT, "tests", "golden", "logei_bounds.json")) as _f:
    BOUNDS = json.load(_f)


def held(metric, err, bar):
    """print, then assert against the hard bar and against 100 × the recorded figure"""
    rec = BOUNDS.get(metric)
    limit = bar if rec is None else min(bar, 100.0 * rec)
    print(f"logei {metric}: achieved {err:.3e} (recorded {rec}, hard bar {bar:.1e})")
    assert err <= limit, f"{metric}: achieved {err:.3e} exceeds {limit:.3e} (hard bar {bar:.1e}, recorded {rec})"


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _score(kind, mu, var, p0, best):
    """abo_score on device copies of mu, var"""
    import torch
    m, v = _dev(mu), _dev(var)
    out = torch.empty_like(m)
    torch.cuda.synchronize()
    abo._lib.check(abo._lib.lib().abo_score(0, m.data_ptr(), v.data_ptr(), m.numel(), kind, float(p0), float(best), out.data_ptr()))
    return out.cpu().numpy()


def _partials(kind, mu, var, p0, best):
    import torch
    m, v = _dev(mu), _dev(var)
    f, a, b = torch.empty_like(m), torch.empty_like(m), torch.empty_like(m)
    torch.cuda.synchronize()
    abo._lib.check(abo._lib.lib().abo_test_acq_partials(0, m.data_ptr(), v.data_ptr(), m.numel(), kind, float(p0), float(best),
                                                        f.data_ptr(), a.data_ptr(), b.data_ptr()))
    return f.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def device_on_golden(golden):
    """(LogEI by abo_score, value / ∂μ / ∂σ² by the refinement's arithmetic, EI by abo_score) over the table's tuples"""
    mu, var, xi, best = golden[:4]
    out = [np.empty_like(mu) for _ in range(5)]
    for x, b in sorted(set(zip(xi, best))):
        s = (xi == x) & (best == b)
        out[0][s] = _score(LOGEI, mu[s], var[s], x, b)
        for o, v in zip(out[1:4], _partials(LOGEI, mu[s], var[s], x, b)):
            o[s] = v
        out[4][s] = _score(EI, mu[s], var[s], x, b)
    return out


def test_score_against_the_mpmath_table(golden, device_on_golden):
    """1.  |got − ref| / max(1, |ref|) over the ≈ 6 400 tuples, −Inf matched exactly, NaN μ → NaN; the partial derivatives relative to
    |ref| (bar: tests/test_logei_cpu.py, PARTIAL_BAR)."""
    ref, rdmu, rdvar = golden[4:]
    got, f, dmu, dvar, _ = device_on_golden
    held("value", value_error(got, ref), VALUE_CEILING)
    np.testing.assert_array_equal(_bits(f), _bits(got))              # acq_score and acq_value_and_partials: one arithmetic
    held("dmu", partial_error(dmu, rdmu), PARTIAL_BAR)
    held("dvar", partial_error(dvar, rdvar), PARTIAL_BAR)
    s = _score(LOGEI, [np.nan, 0.5, np.nan], [1.0, np.nan, 1e-3], 0.0, 0.0)
    assert np.isnan(s).all()
    lib = abo._lib.lib()
    assert lib.abo_score(0, None, None, 0, 9, 0.0, 0.0, None) == 3 and lib.abo_score(0, None, None, 0, 4, 0.0, 0.0, None) == 3
    assert lib.abo_score(0, None, None, 0, LOGEI, 0.0, 0.0, None) == 0


def test_exp_of_logei_is_ei_where_ei_is_representable(golden, device_on_golden):
    """2.  EI's own proved relative error (csrc/misc.hip) is 3.7e-10; LogEI's contributes ≤ 700 · a few · 2⁻⁵³."""
    got, ei = device_on_golden[0], device_on_golden[4]
    ok = ei >= 1e-300
    assert np.sum(ok) > 3000
    err = float(np.max(np.abs(np.exp(got[ok]) / ei[ok] - 1.0)))
    print(f"logei exp(LogEI)/EI - 1: {err:.3e} over {np.sum(ok)} tuples")
    assert err <= 1e-9


ORD = dict(N=64, d=2, M=4096, ell=0.4, sf2=1.0, noise=1e-2, zseed=2)


@pytest.fixture(scope="module")
def ordering():
    N, d, M = ORD["N"], ORD["d"], ORD["M"]
    X, y = synth.standardized_problem(N, d, 0.02)
    Z = synth.points(ORD["zseed"], M, d)
    model = abo.update(make_model(O.MATERN52, ORD["ell"], ORD["sf2"], ORD["noise"]), X, y)
    st = O.fit(O.MATERN52, ORD["ell"], ORD["sf2"], ORD["noise"], 0.0, X, y)
    mu, var = O.predict(st, Z)
    return X, y, Z, model, mu, var


def test_order_is_eis_and_survives_where_ei_underflows(ordering):
    """3.  N = 64, d = 2, M = 4096, Matérn-5/2."""
    X, y, Z, model, mu, var = ordering
    k, best = 32, float(np.min(y))
    _, ev, ei_idx = abo.evaluate(abo.ExpectedImprovement(0.0, best), model, Z, k=k)
    _, lv, li = abo.evaluate(abo.LogExpectedImprovement(0.0, best), model, Z, k=k)
    distinct = (ev > 0.0) & (np.r_[True, ev[1:] != ev[:-1]]) & (np.r_[ev[:-1] != ev[1:], True])
    assert np.sum(distinct) >= k - 2
    np.testing.assert_array_equal(li[distinct], ei_idx[distinct])
    np.testing.assert_allclose(np.exp(lv[distinct]), ev[distinct], rtol=1e-9)
    # ξ so large that z ≤ −40 at every candidate (on the oracle's posterior): EI is 0.0 everywhere
    sg = np.sqrt(var)
    xi = float(np.max(best - mu + 41.0 * sg))
    z = ((best - xi) - mu) / sg
    assert np.all(var > 1e-12) and np.max(z) <= -40.0
    s_ei, ev, ei_idx = abo.evaluate(abo.ExpectedImprovement(xi, best), model, Z, k=k)
    # today's behaviour, and the reason for LogEI: every candidate scores exactly 0 and the stable sort returns the first k
    assert np.all(s_ei == 0.0) and np.all(ev == 0.0)
    np.testing.assert_array_equal(ei_idx, np.arange(k))
    s, lv, li = abo.evaluate(abo.LogExpectedImprovement(xi, best), model, Z, k=k)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(lv))
    ref = logei_restated(mu, var, xi, best)
    err = float(np.max(np.abs(s - ref) / np.maximum(1.0, np.abs(ref))))
    # the device's posterior against the oracle's (δ ≤ 1e-9 in μ and σ²: tests/test_gpu_parity.py) moves LogEI by δ·(Φ/(σh) + φ/(2σ²h)) ≤
    # 1.01·δ·(|z|/σ + z²/(2σ²)) for z ≤ −40, and |ref| ≥ z²/2: relative to |ref| at most 1.01·δ·(2/(|z|σ) + 1/σ²)
    held("ordering_value_vs_oracle", err, 1.01e-9 * float(np.max(2.0 / (np.abs(z) * sg) + 1.0 / var)))
    rec = BOUNDS.get("ordering_value_vs_oracle")
    tol = 100.0 * (rec if rec is not None else err)
    order = np.argsort(-ref, kind="stable")
    top = ref[order[:k + 1]]
    gap = top[:-1] - top[1:]                                        # gap[r]: between ranks r and r + 1 (the last one: to rank k + 1)
    unsure = gap <= 2.0 * tol * np.maximum(1.0, np.abs(top[:-1]))
    unsure = unsure | np.r_[False, unsure[:-1]]
    print(f"logei ordering: smallest top-{k} gap {gap.min():.3e}, excluded {int(np.sum(unsure))}")
    assert np.sum(unsure) <= 2
    np.testing.assert_array_equal(li[~unsure], order[:k][~unsure])
    np.testing.assert_array_equal(_bits(lv), _bits(s[li]))


def test_same_bits_through_every_entry_point(ordering):
    """4.  abo_acq, abo_fit_acq, abo_cand_acq, abo_acq_terms (one term of weight 1), abo_mgpu_acq on a one-device group; a two-term
    ensemble is the fma combination of the single-term scores."""
    X, y, Z, model, mu, var = ordering
    k, best = 16, float(np.min(y))
    for xi in (0.01, float(np.max(best - mu + 41.0 * np.sqrt(var)))):
        acq = abo.LogExpectedImprovement(xi, best)
        s, tv, ti = abo.evaluate(acq, model, Z, k=k)
        assert np.all(np.isfinite(s))
        fresh = make_model(O.MATERN52, ORD["ell"], ORD["sf2"], ORD["noise"])
        _, s1, tv1, ti1 = abo.update_and_evaluate(acq, fresh, X, y, Z, k=k, best_y=best)
        s2, tv2, ti2 = abo.ResidentCandidates(model, Z).evaluate(acq, k=k, return_scores=True)
        s3, tv3, ti3 = A.evaluate_terms([(LOGEI, xi, best, 1.0)], model, Z, k=k)
        group = abo.update(abo.HipShardedGP(ORD["sf2"] * abo.with_lengthscale(abo.Matern52Kernel(), ORD["ell"]), ORD["noise"], devices=(0,)),
                           X, y)
        s4, tv4, ti4 = abo.evaluate(acq, group, Z, k=k)
        for name, (a, b, c) in {"abo_fit_acq": (s1, tv1, ti1), "abo_cand_acq": (s2, tv2, ti2), "abo_acq_terms": (s3, tv3, ti3),
                                "abo_mgpu_acq": (s4, tv4, ti4)}.items():
            assert np.array_equal(_bits(a), _bits(s)), name
            assert np.array_equal(_bits(b), _bits(tv)) and np.array_equal(c, ti), name
        ucb, _, _ = abo.evaluate(abo.UpperConfidenceBound(2.0), model, Z, k=0)
        ens, _, _ = A.evaluate_terms([(LOGEI, xi, best, 0.5), (UCB, 2.0, 0.0, 0.5)], model, Z, k=0)
        np.testing.assert_array_equal(_bits(ens), _bits(0.5 * ucb + 0.5 * s))      # fma(½, ucb, ½·logei): ½·x is exact, one rounding
    lib = abo._lib.lib()
    bad = lib.abo_acq(model._require(), Z.ctypes.data, 4, ORD["d"], 0, 9, 0.0, 0.0, 0, None, 0, None, None, 0)
    assert bad == 3                                                              # ABO_EINVAL


def _fd4(fun, Z, h):
    n, d = Z.shape
    pts = np.repeat(Z[:, None, :], 4 * d, axis=1)
    for c in range(d):
        for q, mult in enumerate((2.0, 1.0, -1.0, -2.0)):
            pts[:, 4 * c + q, c] += mult * h
    vals = fun(pts.reshape(-1, d)).reshape(n, 4 * d)
    return (-vals[:, 0::4] + 8.0 * vals[:, 1::4] - 8.0 * vals[:, 2::4] + vals[:, 3::4]) / (12.0 * h)


def _acq_grad(model, kind, p0, best, Z):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    f, g = np.empty(Z.shape[0]), np.empty(Z.shape)
    abo._lib.check(abo._lib.lib().abo_test_acq_grad(model._require(), kind, float(p0), float(best), Z.ctypes.data, Z.shape[0], Z.shape[1],
                                                    f.ctypes.data, g.ctypes.data))
    return f, g


def test_gradient_against_central_differences_of_the_restatement():
    """5.  N = 32, d = 3, 64 points: 60 under a noisy model (σ of a few tenths: LogEI is smooth over the stencil), with ξ set so that one
    of them sits at z = −1, −64, −200 in turn (every range of log_h and both seams' neighbourhoods), and 4 training points of a
    noise-free model (σ² = 1e-18 ≤ 1e-12: the degenerate branch).  Bar: 2e-5 relative, as tests/test_gpu_refine.py."""
    N, d = 32, 3
    X, y = synth.standardized_problem(N, d, 0.03)
    ell, sf2, noise = 0.7 * np.sqrt(d), 1.3, 0.1
    m = abo.update(make_model(O.MATERN52, ell, sf2, noise), X, y)
    st = O.fit(O.MATERN52, ell, sf2, noise, 0.0, X, y)
    Z = synth.points(5, 60, d) * 2.0 - 0.5
    best = float(np.median(y))
    mu, var = O.predict(st, Z)
    for j, target in ((7, -1.0), (23, -64.0), (41, -200.0)):
        xi = float(best - mu[j] - target * np.sqrt(var[j]))
        z = ((best - xi) - mu) / np.sqrt(var)
        assert abs(z[j] - target) < 1e-9 * abs(target) and np.all(var > 1e-12)
        print(f"logei gradient: target z = {target}: z over the points {z.min():.1f} … {z.max():.1f}")
        f, g = _acq_grad(m, LOGEI, xi, best, Z)
        oracle = lambda p: logei_restated(*O.predict(st, p), xi, best)
        ref = oracle(Z)
        assert np.max(np.abs(f - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-8
        fd = _fd4(oracle, Z, 2e-5)
        scale = np.maximum(np.max(np.abs(fd), axis=1, keepdims=True), 1e-3)
        assert np.percentile(np.max(np.abs(fd), axis=1), 50) > 1e-3
        err = float(np.max(np.abs(g - fd) / scale))
        print(f"logei gradient: target z = {target}: rel. error against oracle central differences {err:.3e}")
        assert err <= 2e-5
    # the degenerate branch: value log Δ, gradient −∇μ/Δ where Δ > 0; −Inf and 0 where Δ ≤ 0
    m0 = abo.update(make_model(O.MATERN52, 0.5, 1.0, 0.0), X, y)
    st0 = O.fit(O.MATERN52, 0.5, 1.0, 0.0, 0.0, X, y)
    P = X[:4].copy()
    assert np.all(abo.posterior_var(m0, P) <= 1e-12)
    xi = float(-np.sort(y[:4])[1] - 0.5 * (np.sort(y[:4])[2] - np.sort(y[:4])[1]))    # best = 0: Δ = −ξ − y > 0 at two of them
    f, g = _acq_grad(m0, LOGEI, xi, 0.0, P)
    delta = -xi - y[:4]
    pos = delta > 0
    assert np.sum(pos) == 2
    np.testing.assert_allclose(f[pos], np.log(delta[pos]), atol=1e-8)
    gmu = _fd4(lambda p: O.predict(st0, p)[0], P, 2e-5)
    scale = np.maximum(np.max(np.abs(gmu[pos] / delta[pos, None]), axis=1, keepdims=True), 1e-3)
    assert float(np.max(np.abs(g[pos] + gmu[pos] / delta[pos, None]) / scale)) <= 2e-5
    assert np.all(np.isneginf(f[~pos])) and np.all(g[~pos] == 0.0)


def test_refinement_where_eis_does_not_start():
    """6.  N = 32, d = 2, 8 starts, ξ such that z ≤ −8 (EI < 1e-12) at every start."""
    from scipy.optimize import minimize
    N, d, S = 32, 2, 8
    X, y = synth.standardized_problem(N, d, 0.02)
    ell, sf2, noise = 0.5, 1.0, 0.05
    m = abo.update(make_model(O.MATERN52, ell, sf2, noise), X, y)
    st = O.fit(O.MATERN52, ell, sf2, noise, 0.0, X, y)
    lower, upper = np.full(d, -0.5), np.full(d, 1.5)
    starts = synth.points(7, S, d) * 2.0 - 0.5
    best = float(np.min(y))
    mu, var = O.predict(st, starts)
    xi = float(np.max(best - mu + 8.0 * np.sqrt(var)))
    assert np.max(O.expected_improvement(mu, var, best, xi)) < 1e-12
    lib = abo._lib.lib()
    st_c, lo_c, up_c = np.ascontiguousarray(starts), np.ascontiguousarray(lower), np.ascontiguousarray(upper)

    def refine(kind):
        x, f, it = np.empty((S, d)), np.empty(S), np.zeros((S, 2), dtype=np.int32)
        abo._lib.check(lib.abo_refine(m._require(), kind, xi, best, lo_c.ctypes.data, up_c.ctypes.data, d, st_c.ctypes.data, S, None,
                                      x.ctypes.data, f.ctypes.data, it.ctypes.data))
        return x, f, it

    xe, fe, ite = refine(EI)
    print(f"logei refine: EI from the same starts: values {fe.max():.3e}, iterations {ite[:, 0]}")
    assert np.all(ite[:, 0] == 0) and np.array_equal(xe, starts) and np.all(fe < 1e-12)      # today's behaviour: nothing moves
    xr, fr, it = refine(LOGEI)
    f0, _ = _acq_grad(m, LOGEI, xi, best, starts)
    acq = abo.LogExpectedImprovement(xi, best)
    print(f"logei refine: start values {f0}, refined {fr}, iterations {it[:, 0]}, evaluations {it[:, 1]}")
    assert np.all(np.isfinite(f0)) and np.all(fr >= f0 - 1e-12)          # (f0: another launch's summation of the same value)
    assert np.all(xr >= lower) and np.all(xr <= upper)
    np.testing.assert_allclose(acq(m, xr), fr, rtol=0.0, atol=1e-9)
    assert np.sum(fr - f0 > 2.2e-9) >= S // 2 and np.all(it[:, 0] <= 100)
    oracle = lambda p: logei_restated(*O.predict(st, p), xi, best)
    fs_best = -np.inf
    for i in range(S):
        res = minimize(lambda p: -float(oracle(p[None, :])[0]), starts[i], method="L-BFGS-B", bounds=list(zip(lower, upper)),
                       options={"ftol": 1e-14, "gtol": 1e-8})
        fs_best = max(fs_best, -res.fun)
    short = max(0.0, fs_best - float(np.max(fr))) / max(1.0, abs(fs_best))
    print(f"logei refine: best of starts {np.max(fr):.9f}, SciPy on the restatement {fs_best:.9f}, shortfall {short:.3e}")
    assert short <= 1e-5                       # the bar of tests/test_gpu_refine.py's small cases (best_of_starts_shortfall_rel)
    bx, bv, sx, sv, rx, rv = A.optimize_acquisition_device(acq, m, abo.ContinuousDomain(lower, upper), n_grid=2000, n_local=8, seed=3,
                                                           return_all=True)
    print(f"logei optimize_acquisition: best grid score {np.max(sv):.6f}, returned {bv:.6f}")
    assert np.isfinite(bv) and bv >= np.max(sv) and np.all(bx >= lower) and np.all(bx <= upper)


def _force(rblocks, mode):
    abo._lib.check(abo._lib.lib().abo_test_prune_force(rblocks, mode))


def test_pruned_selection_returns_the_full_evaluations_pairs():
    """7.  N = 1536, d = 8, M = 20 000, k = 16, int8 engine: the shape of tests/test_gpu_acq_prune.py's typical case."""
    N, d, M, k = 1536, 8, 20000, 16
    X, y = synth.standardized_problem(N, d, 0.03)
    Z = synth.points(2, M, d)
    model = abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8"), X, y)
    best = float(np.min(y))
    ei, logei = abo.ExpectedImprovement(0.01, best), abo.LogExpectedImprovement(0.01, best)

    def bounds():
        ub = np.empty(M)
        abo._lib.check(abo._lib.lib().abo_test_prune_bounds(model._require(), ub.ctypes.data, M))
        return ub

    def expected_survivors(ub, s, abs_margin, k0=1024):
        """the compaction's count restated: threshold = the k-th best exact score among the k0 best by bound, kept = not (guard < it)"""
        first = np.lexsort((np.arange(M), -ub))[:k0]
        tau = np.sort(s[first])[::-1][k - 1]
        return int(np.sum(~(ub + np.abs(ub) * PRUNE_REL + abs_margin < tau)))

    try:
        _force(0, 0)
        _, ev, ei_i = abo.evaluate(ei, model, Z, k=k, return_scores=False)
        st_ei = model.prune_stats()
        ub_ei = bounds()
        _, lv, li = abo.evaluate(logei, model, Z, k=k, return_scores=False)
        st = model.prune_stats()
        ub = bounds()
        print(f"logei prune: EI {st_ei}\nlogei prune: LOGEI {st}")
        assert st["pruned"] == 1 and st["fallback"] == 0 and st["bound_rows"] == 256 and st["k0"] == 1024
        assert model.timings()["contraction_engine"] == abo._lib.CONTRACT_INT8
        _, ev2, ei_i2 = abo.evaluate(ei, model, Z, k=k, return_scores=False)
        st_ei2 = model.prune_stats()
        # EI's count is that of its own guard, ub·(1 + 2⁻³⁰) + 2⁻¹⁰²², before and after a LOGEI call
        s_ei, _, _ = abo.evaluate(ei, model, Z, k=0)
        assert st_ei["pruned"] == 1 and st_ei2["survivors"] == st_ei["survivors"] == expected_survivors(ub_ei, s_ei, PRUNE_ABS)
        assert np.array_equal(_bits(ev2), _bits(ev)) and np.array_equal(ei_i2, ei_i)
        s, _, _ = abo.evaluate(logei, model, Z, k=0)
        assert model.prune_stats()["bound_rows"] == 0
        assert st["survivors"] == expected_survivors(ub, s, PRUNE_ABS_LOGEI)
        # bound dominance: the guarded bound of every candidate is at least its exact score
        slack = ub + np.abs(ub) * PRUNE_REL + PRUNE_ABS_LOGEI - s
        print(f"logei prune: min(guarded bound - score) = {slack.min():.3e}, bound > score on {np.mean(ub > s):.4f} of the candidates")
        assert np.all(slack >= 0.0)
        ov, oi = O.top_k(s, k)
        assert np.array_equal(li, oi) and np.array_equal(_bits(lv), _bits(s[oi]))
        np.testing.assert_array_equal(li, ei_i)                        # and EI's order, all 16 being positive and distinct
        for mode in (2, 1):                                            # the path off; a threshold of −Inf (every candidate survives)
            _force(0, mode)
            _, lv_m, li_m = abo.evaluate(logei, model, Z, k=k, return_scores=False)
            stm = model.prune_stats()
            assert (stm["bound_rows"] == 0) if mode == 2 else (stm["survivors"] == M and stm["fallback"] == 1)
            assert np.array_equal(_bits(lv_m), _bits(lv)) and np.array_equal(li_m, li), mode
    finally:
        _force(0, 0)
