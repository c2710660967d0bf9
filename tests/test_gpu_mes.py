"""GPU tests (-m gpu) of max-value entropy search (ABO_ACQ_MES = 6; csrc/abo_acq_dev.h: mes_a): the device arithmetic
against the mpmath table tests/golden/mes_kat.npz, the same bits through every entry point, the selection, the analytic gradient, the
refinement, the samples from the Thompson paths, and the refusals.

The CPU restatement of MES (tests/test_mes_cpu.py: mes_restated) on the oracle's posterior is the reference wherever a model is involved.
Achieved errors of the device arithmetic are DATA in tests/golden/mes_bounds.json, measured on an MI355X by this file: every GPU
session leaves them under the case "mes" of the suite's record of achieved errors (tests/parity_record.py: OUT_PATH), from where they
are copied.  A figure is asserted at 100 × its recorded value and at its hard bar: 1e-12 for the value, for the partial derivatives
the bar of the restatement (tests/test_mes_cpu.py: PARTIAL_BAR, derived there from the two cancellations of the erfcx range)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import acquisition as A
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

from tests import parity_record
from tests.test_gpu_parity import make_model
from tests.test_mes_cpu import (PARTIAL_BAR, check_tail_partials, gamma_extremes, group_samples, load_golden, mes_restated, over_groups, partial_error,
                                value_error)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MES, EINVAL = 6, 3
VALUE_CEILING = 1e-12                  # |got − ref| ≤ 1e-12·max(1, |ref|): LogEI's ceiling (the same functions: erfcx, log1p, log)

with open(os.path.join(ROOT, "tests", "golden", "mes_bounds.json")) as _f:
    BOUNDS = json.load(_f)


def held(metric, err, bar):
    """print, record and hold to the hard bar (parity_record.check: case "mes" of the suite's record), then to 100 × the recorded figure"""
    rec = BOUNDS[metric]
    print(f"mes {metric}: achieved {err:.3e} (recorded {rec}, hard bar {bar})")
    parity_record.check("mes", metric, err, bar, tighten=False)
    limit = min(bar, 100.0 * rec)
    assert err <= limit, f"{metric}: achieved {err:.3e} exceeds {limit:.3e} (hard bar {bar}, recorded {rec})"


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _score(mu, var, ystar, ys_device=False):
    """abo_score_mes on device copies of mu, var (the samples from host memory, or from a device copy)"""
    import torch
    m, v = _dev(mu), _dev(var)
    ys = np.ascontiguousarray(ystar, dtype=np.float64)
    yd = _dev(ys) if ys_device else None
    out = torch.empty_like(m)
    torch.cuda.synchronize()
    abo._lib.check(abo._lib.lib().abo_score_mes(0, m.data_ptr(), v.data_ptr(), m.numel(), yd.data_ptr() if ys_device else ys.ctypes.data,
                                                len(ys), 1 if ys_device else 0, out.data_ptr()))
    return out.cpu().numpy()


def _partials(mu, var, ystar):
    import torch
    m, v, ys = _dev(mu), _dev(var), _dev(ystar)
    f, a, b = torch.empty_like(m), torch.empty_like(m), torch.empty_like(m)
    torch.cuda.synchronize()
    abo._lib.check(abo._lib.lib().abo_test_mes_partials(0, m.data_ptr(), v.data_ptr(), m.numel(), ys.data_ptr(), ys.numel(),
                                                        f.data_ptr(), a.data_ptr(), b.data_ptr()))
    return f.cpu().numpy(), a.cpu().numpy(), b.cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_score_against_the_mpmath_table(golden):
    """4.  |got − ref| / max(1, |ref|) over the table; samples from host and from device memory give the same bits; NaN → NaN."""
    got = over_groups(golden, lambda m, v, ys: (_score(m, v, ys),) * 3)[0]
    held("value", value_error(got, golden["mes"]), VALUE_CEILING)
    assert np.all(got >= 0.0)
    g = int(np.argmax(np.diff(golden["goff"]) == 16))
    s = golden["grp"] == g
    np.testing.assert_array_equal(_bits(_score(golden["mu"][s], golden["var"][s], group_samples(golden, g), ys_device=True)), _bits(got[s]))
    ys = np.array([-1.0, 0.5])
    assert np.isnan(_score([np.nan, 0.5, np.nan], [1.0, np.nan, 0.0], ys)).all()
    assert np.all(_score([0.3, np.inf, -7.0], [1e-12, 0.0, 1e-13], ys) == 0.0)          # degenerate variance; an excluded candidate


def test_partials_against_the_mpmath_table(golden):
    """5.  relative error of ∂/∂μ, ∂/∂σ² for γ ≥ −64; below, finiteness and sign."""
    f, dmu, dvar = over_groups(golden, _partials)
    assert value_error(f, golden["mes"]) <= VALUE_CEILING
    lo, hi = gamma_extremes(golden)
    body = (golden["var"] > 1e-12) & (lo >= -64.0)
    held("dmu", partial_error(dmu, golden["dmu"], body), PARTIAL_BAR)
    held("dvar", partial_error(dvar, golden["dvar"], body), PARTIAL_BAR)
    tail = check_tail_partials(golden, dmu, dvar)
    assert np.all(dmu <= 0.0)                                                    # non-increasing in μ everywhere
    neg = (golden["var"] > 1e-12) & (hi < 0.0)                                   # ∂/∂σ² has the sign of −γ·a'(γ): every γ < 0 → < 0
    pos = (golden["var"] > 1e-12) & (lo > 0.0)
    assert np.all(dvar[neg] < 0.0) and np.all(dvar[pos] >= 0.0) and np.sum(tail & neg) == np.sum(tail)


E = dict(N=200, d=3, M=3000, S=16, ell=0.6, sf2=1.0, noise=1e-2)


@pytest.fixture(scope="module")
def entry():
    N, d, M = E["N"], E["d"], E["M"]
    X, y = synth.standardized_problem(N, d, 0.02)
    Z = synth.points(2, M, d)
    Z[20, 1] = np.nan                      # one NaN coordinate: NaN score, ranked first
    model = abo.update(make_model(O.MATERN52, E["ell"], E["sf2"], E["noise"]), X, y)
    ystar = float(np.min(y)) - 0.05 * np.arange(E["S"])
    # two duplicated candidates, placed where the selection sees them: copies of the best and of the 100th candidate, each in the
    # slot behind its original — ties, kept in index order
    first = O.top_k(abo.MaxValueEntropySearch(ystar)(model, Z), 100)[1]
    dup = [int(first[1]), int(first[99])]
    assert all(j + 1 < M and j + 1 != 20 and j != 20 for j in dup) and abs(dup[0] - dup[1]) > 1
    for j in dup:
        Z[j + 1] = Z[j]
    return X, y, Z, model, ystar, dup


def _order(scores, k, idx_base):
    ov, oi = O.top_k(scores, min(k, len(scores)))
    return ov, oi + idx_base


def test_same_bits_through_every_entry_point(entry):
    """6.  N = 200, d = 3, M = 3000, S = 16, Matérn-5/2."""
    X, y, Z, model, ystar, dup = entry
    acq = abo.MaxValueEntropySearch(ystar)
    M, base = E["M"], 70000
    mu, var = abo.mean_and_var(model, Z)
    ref = _score(mu, var, ystar)
    assert np.isnan(ref[20]) and np.sum(np.isnan(ref)) == 1
    cands = abo.ResidentCandidates(model, Z)
    cands.exclude(333)
    ref_c = ref.copy()
    ref_c[333] = 0.0                                                             # stored μ = +Inf, σ² = 0
    for k in (7, 1500):
        s, tv, ti = abo.evaluate(acq, model, Z, k=k, idx_base=base)
        np.testing.assert_array_equal(_bits(s), _bits(ref))
        assert all(v == 0 for v in model.prune_stats().values()), model.prune_stats()
        s2, tv2, ti2 = abo.evaluate(acq, model, Z, k=k, idx_base=base)
        assert np.array_equal(_bits(s2), _bits(s)) and np.array_equal(_bits(tv2), _bits(tv)) and np.array_equal(ti2, ti)
        ov, oi = _order(s, k, base)
        np.testing.assert_array_equal(ti, oi)
        np.testing.assert_array_equal(_bits(tv), _bits(ov))
        assert ti[0] == base + 20 and np.isnan(tv[0])
        sc, tvc, tic = cands.evaluate(acq, k=k, idx_base=base, return_scores=True)
        np.testing.assert_array_equal(_bits(sc), _bits(ref_c))
        ov, oi = _order(sc, k, base)
        np.testing.assert_array_equal(tic, oi)
        np.testing.assert_array_equal(_bits(tvc), _bits(ov))
        # without the scores (the call the pruned selection would take for EI): the same pairs, and no pruning
        _, tv3, ti3 = abo.evaluate(acq, model, Z, k=k, idx_base=base, return_scores=False)
        assert np.array_equal(_bits(tv3), _bits(tv)) and np.array_equal(ti3, ti)
        assert all(v == 0 for v in model.prune_stats().values())
    where = {int(i): r for r, i in enumerate(ti - base)}                         # (k = 1500: both duplicated pairs are in)
    for j in dup:
        assert where[j] + 1 == where[j + 1] and s[j] == s[j + 1], j
    # the (NaN, −1) tail when k exceeds M
    few = Z[:5]
    s5, tv5, ti5 = abo.evaluate(acq, model, few, k=8, idx_base=3)
    assert np.all(ti5[5:] == -1) and np.isnan(tv5[5:]).all() and np.array_equal(np.sort(ti5[:5]), 3 + np.arange(5))
    # a CUDA tensor of candidates: the same bits, outputs on the device
    import torch
    sd, tvd, tid = abo.evaluate(acq, model, torch.from_numpy(Z).cuda(), k=7)
    assert sd.is_cuda and np.array_equal(_bits(sd.cpu().numpy()), _bits(ref)) and np.array_equal(tid.cpu().numpy() + base, abo.evaluate(acq, model, Z, k=7, idx_base=base)[2])
    # against the restatement on the oracle's posterior
    st = O.fit(O.MATERN52, E["ell"], E["sf2"], E["noise"], 0.0, X, y)
    omu, ovar = O.predict(st, Z)
    ok = ~np.isnan(ref)
    err = float(np.max(np.abs(ref[ok] - mes_restated(omu[ok], ovar[ok], ystar)) / np.maximum(1.0, ref[ok])))
    print(f"mes entry points: against the restatement on the oracle's posterior {err:.3e}")
    assert err <= 1e-6


def _fd4(fun, Z, h):
    from tests.test_gpu_refine import _fd4 as fd4
    return fd4(fun, Z, h)


def test_gradient_against_central_differences_of_the_restatement():
    """7.  N = 64, d = 3, 32 points under a noisy model — 8 training points, 12 in the box, 12 far outside the data — with samples around
    the targets' median (γ of both signs and moderate size, so that MES varies over the points: with samples at the data's minimum and
    this much noise γ is large and MES flat 0 at most of them) and with samples far ABOVE every mean (γ from −25 down: the erfcx range and the series), and 4 training points
    of a noise-free model (σ² = 1e-18 ≤ 1e-12: the degenerate branch, value and gradient exactly 0).  Step 2e-5 and bar 2e-5 relative
    to the point's largest component (floor 1e-3), as tests/test_gpu_refine.py's gradient check."""
    N, d = 64, 3
    X, y = synth.standardized_problem(N, d, 0.03)
    ell, sf2, noise = 0.7 * np.sqrt(d), 1.3, 0.1
    m = abo.update(make_model(O.MATERN52, ell, sf2, noise), X, y)
    st = O.fit(O.MATERN52, ell, sf2, noise, 0.0, X, y)
    Z = np.vstack([X[:8], synth.points(5, 12, d), synth.points(6, 12, d) * 8.0 - 4.0])
    assert len(Z) == 32
    mu, var = O.predict(st, Z)
    assert np.all(var > 1e-12)
    h = 2e-5
    for name, ystar in (("around_the_median", float(np.median(y)) + 0.05 * (np.arange(16) - 8.0)), ("far_above", 25.0 + 0.5 * np.arange(16))):
        g_lo = (mu - ystar.max()) / np.sqrt(var)
        print(f"mes gradient {name}: γ over the points {g_lo.min():.1f} … {((mu - ystar.min()) / np.sqrt(var)).max():.1f}")
        acq = abo.MaxValueEntropySearch(ystar)
        f, g = A.acquisition_value_and_grad(acq, m, Z)
        np.testing.assert_allclose(f, acq(m, Z), rtol=1e-9, atol=1e-10)       # the scored path's value (another summation order)
        oracle = lambda p: mes_restated(*O.predict(st, p), ystar)
        np.testing.assert_allclose(f, oracle(Z), rtol=1e-8, atol=1e-11)
        fd = _fd4(oracle, Z, h)
        scale = np.maximum(np.max(np.abs(fd), axis=1, keepdims=True), 1e-3)
        assert np.percentile(np.max(np.abs(fd), axis=1), 50) > 1e-3
        err = float(np.max(np.abs(g - fd) / scale))
        print(f"mes gradient {name}: rel. error against oracle central differences {err:.3e}")
        assert err <= 2e-5
    assert g_lo.min() < -64.0 and g_lo.max() > -32.0                             # (far_above reaches both negative ranges)
    m0 = abo.update(make_model(O.MATERN52, 0.5, 1.0, 0.0), X, y)
    P = X[:4].copy()
    assert np.all(abo.posterior_var(m0, P) <= 1e-12)
    f, g = A.acquisition_value_and_grad(abo.MaxValueEntropySearch([-3.0, 2.0]), m0, P)
    assert np.all(f == 0.0) and np.all(g == 0.0)


def test_refinement_against_scipy_on_the_restatement():
    """8.  N = 40, d = 2, 16 starts, S = 16: the three properties and the bars of tests/test_gpu_refine.py (its _against_scipy)."""
    from tests.test_gpu_refine import _against_scipy
    N, d, S = 40, 2, 16
    X, y = synth.standardized_problem(N, d, 0.02)
    ell, sf2, noise = 0.5, 1.0, 0.05
    m = abo.update(make_model(O.MATERN52, ell, sf2, noise), X, y)
    st = O.fit(O.MATERN52, ell, sf2, noise, 0.0, X, y)
    lower, upper = np.full(d, -0.5), np.full(d, 1.5)
    dom = abo.ContinuousDomain(lower, upper)
    grid = abo.latin_hypercube(2000, lower, upper, np.random.default_rng(4))
    ystar = abo.max_value_samples(m, grid, S, R=512, rng=9)
    acq = abo.MaxValueEntropySearch(ystar)
    starts = synth.points(7, 16, d) * 2.0 - 0.5
    f0 = acq(m, starts)
    xr, fr, it = abo.refine_starts(acq, m, starts, lower, upper, return_iters=True)
    print(f"mes refine: samples {ystar.min():.3f} … {ystar.max():.3f}; start values {f0.min():.4f} … {f0.max():.4f}, refined "
          f"{fr.min():.4f} … {fr.max():.4f}, iterations {it[:, 0]}")
    assert np.all(fr >= f0 - 1e-15), "a refined start lost against its start"
    assert np.all(xr >= lower) and np.all(xr <= upper)
    np.testing.assert_allclose(acq(m, xr), fr, rtol=1e-9, atol=1e-10)
    assert np.all(it[:, 0] <= 100) and np.all(it[:, 1] <= 1 + (2 * 100 + 2) * 20)
    assert it[:, 1].sum() > 3 * len(starts) and np.sum(fr - f0 > 2.2e-9) >= len(starts) // 2      # (not vacuous: most starts climb)
    oracle = lambda p: mes_restated(*O.predict(st, p), ystar)
    _against_scipy("refine/mes_d2_N40", "MaxValueEntropySearch", oracle,
                   lambda **kw: abo.refine_starts(acq, m, starts, lower, upper, **kw), starts, xr, fr, lower, upper)
    # the one call: its starts are abo_acq_mes's top n_local over abo_lhs's grid, it returns the best of its refined values
    n_grid, n_local, seed = 2000, 8, 3
    bx, bv, sx, sv, rx, rv = A.optimize_acquisition_device(acq, m, dom, n_grid=n_grid, n_local=n_local, seed=seed, return_all=True)
    lhs = abo.device_latin_hypercube(n_grid, lower, upper, seed, m.device)
    _, tv, ti = abo.evaluate(acq, m, lhs, k=n_local, return_scores=False)
    np.testing.assert_array_equal(_bits(sv), _bits(tv.cpu().numpy()))
    np.testing.assert_array_equal(sx, lhs[ti].cpu().numpy())
    xr2, fr2 = abo.refine_starts(acq, m, sx, lower, upper)
    np.testing.assert_array_equal(_bits(rv), _bits(fr2))
    np.testing.assert_array_equal(rx, xr2)
    j = int(np.argmax(rv))
    assert np.all(np.isfinite(rv)) and rv[j] >= sv[0] and bv == rv[j] and np.array_equal(bx, rx[j])
    assert np.all(bx >= lower) and np.all(bx <= upper)

def test_lockstep_refinement_equals_the_one_launch_kernel_to_rounding(monkeypatch):
    """8b.  From 1024 factor rows on the refinement runs in lockstep rounds (csrc/refine.hip: rl_reduce_kernel, its MES instantiation);
    forced here at N = 200 (ABO_REFINE_LOCKSTEP_NP), d = 3, 24 starts, S = 16, as tests/test_gpu_refine.py does for EI and UCB and
    with its bars: both variants land on the same value for at least nine starts in ten (1e-6 relative), none loses against its
    start, all stay in the box, the reported value is the score of the reported point, two runs give the same bits."""
    N, d, S = 200, 3, 24
    X, y = synth.standardized_problem(N, d, 0.02)
    ell, sf2, noise = 0.5, 1.0, 0.05
    m = abo.update(make_model(O.MATERN52, ell, sf2, noise, n_max=N + 8), X, y)
    st = O.fit(O.MATERN52, ell, sf2, noise, 0.0, X, y)
    lower, upper = np.full(d, -0.5), np.full(d, 1.5)
    ystar = float(np.median(y)) + 0.05 * (np.arange(16) - 8.0)
    acq = abo.MaxValueEntropySearch(ystar)
    starts = synth.points(11, S, d) * 2.0 - 0.5
    f0 = acq(m, starts)
    monkeypatch.setenv("ABO_REFINE_LOCKSTEP_NP", "0")
    xa, fa, ita = abo.refine_starts(acq, m, starts, lower, upper, return_iters=True)
    monkeypatch.setenv("ABO_REFINE_LOCKSTEP_NP", "128")
    xb, fb, itb = abo.refine_starts(acq, m, starts, lower, upper, return_iters=True)
    xb2, fb2 = abo.refine_starts(acq, m, starts, lower, upper)
    np.testing.assert_array_equal(_bits(fb), _bits(fb2))
    np.testing.assert_array_equal(xb, xb2)
    assert np.all(np.isfinite(fa)) and np.all(np.isfinite(fb))
    assert np.all(fb >= f0 - 1e-10) and np.all(xb >= lower) and np.all(xb <= upper)
    np.testing.assert_allclose(acq(m, xb), fb, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(mes_restated(*O.predict(st, xb), ystar), fb, rtol=1e-7, atol=1e-9)
    close = np.abs(fa - fb) <= 1e-6 * np.maximum(1.0, np.abs(fa))
    print(f"mes lockstep: one launch {fa.min():.4f} … {fa.max():.4f}, lockstep {fb.min():.4f} … {fb.max():.4f}, equal on {close.mean():.2f} "
          f"of the starts, evaluations {itb[:, 1].sum()} (one launch {ita[:, 1].sum()}), median gain {np.median(fb - f0):.3e}")
    assert close.mean() >= 0.9
    assert itb[:, 1].sum() > 2 * S and np.all(itb[:, 0] <= 100) and np.sum(fb - f0 > 2.2e-9) >= S // 2


def test_samples_end_to_end():
    """9.  a 2000-point grid, S = 8."""
    N, d, M, S, R = 96, 2, 2000, 8, 256
    X, y = synth.standardized_problem(N, d, 0.02)
    m = abo.update(make_model(O.MATERN52, 0.5, 1.0, 1e-3), X, y)
    Z = synth.points(3, M, d)
    ys = abo.max_value_samples(m, Z, S, R=R, rng=11)
    tv, ti = abo.sample_paths(m, S, R, rng=11).argmin(Z, k=1)
    assert ys.shape == (S,) and np.array_equal(_bits(ys), _bits(tv[:, 0]))
    vals = abo.sample_paths(m, S, R, rng=11)(Z)
    np.testing.assert_allclose(ys, vals.min(axis=1), rtol=0.0, atol=1e-9)       # (the values pass: another launch)
    ysc = abo.max_value_samples(m, abo.ResidentCandidates(m, Z), S, R=R, rng=11)
    np.testing.assert_allclose(ysc, ys, rtol=0.0, atol=1e-9)
    s = abo.MaxValueEntropySearch(ys)(m, Z)
    _, var = abo.mean_and_var(m, Z)
    assert np.all(np.isfinite(s[var > 1e-12])) and np.all(s >= 0.0) and np.max(s) > 0.0
    print(f"mes samples: y* {ys.min():.3f} … {ys.max():.3f} (min y {y.min():.3f}); MES up to {s.max():.4f}")


def test_refusals_leave_the_handle_usable(entry):
    """10.  every refusal is ABO_EINVAL with a reason, and the handle scores afterwards."""
    X, y, Z, model, ystar, _ = entry
    L, h, d = abo._lib.lib(), model._require(), E["d"]
    few = np.ascontiguousarray(Z[:4])
    out = np.empty(4)
    ys = np.ascontiguousarray(ystar)
    big = np.zeros(1025)
    bad = ys.copy()
    bad[3] = np.nan

    def acq_mes(p, n):
        return L.abo_acq_mes(h, few.ctypes.data, 4, d, 0, p, n, 0, 0, out.ctypes.data, 0, None, None, 0)

    lo, up = np.zeros(d), np.ones(d)
    xo, fo = np.empty((4, d)), np.empty(4)
    bx, bv = np.empty(d), C.c_double()
    cands = abo.ResidentCandidates(model, few)
    calls = {
        "S = 0": lambda: acq_mes(ys.ctypes.data, 0),
        "S = 1025": lambda: acq_mes(big.ctypes.data, 1025),
        "NaN sample": lambda: acq_mes(bad.ctypes.data, len(bad)),
        "null ystar": lambda: acq_mes(None, 4),
        "score S = 0": lambda: L.abo_score_mes(0, None, None, 0, ys.ctypes.data, 0, 0, None),
        "score null": lambda: L.abo_score_mes(0, None, None, 0, None, 4, 0, None),
        "cand S = 1025": lambda: L.abo_cand_acq_mes(h, cands._h.ptr, big.ctypes.data, 1025, 0, 0, out.ctypes.data, 0, None, None, 0),
        "cand NaN": lambda: L.abo_cand_acq_mes(h, cands._h.ptr, bad.ctypes.data, len(bad), 0, 0, out.ctypes.data, 0, None, None, 0),
        "refine NaN": lambda: L.abo_refine_mes(h, bad.ctypes.data, len(bad), lo.ctypes.data, up.ctypes.data, d, few.ctypes.data, 4, None,
                                               xo.ctypes.data, fo.ctypes.data, None),
        "refine S = 0": lambda: L.abo_refine_mes(h, ys.ctypes.data, 0, lo.ctypes.data, up.ctypes.data, d, few.ctypes.data, 4, None,
                                                 xo.ctypes.data, fo.ctypes.data, None),
        "optimize null": lambda: L.abo_optimize_acquisition_mes(h, None, 4, lo.ctypes.data, up.ctypes.data, d, 100, 4, 1, None,
                                                                bx.ctypes.data, C.byref(bv), None, None, None, None),
        "kind 6 in abo_acq": lambda: L.abo_acq(h, few.ctypes.data, 4, d, 0, MES, 0.0, 0.0, 0, out.ctypes.data, 0, None, None, 0),
        "kind 6 in abo_score": lambda: L.abo_score(0, None, None, 0, MES, 0.0, 0.0, None),
        "kind 6 in abo_acq_terms": lambda: L.abo_acq_terms(h, few.ctypes.data, 4, d, 0, A._term_array([(MES, 0.0, 0.0, 1.0)]), 1, 0,
                                                           out.ctypes.data, 0, None, None, 0),
    }
    want = abo.MaxValueEntropySearch(ystar)(model, few)
    for name, call in calls.items():
        assert call() == EINVAL, name
        msg = abo._lib.last_error()
        assert len(msg) > 10, name
        if name.startswith("kind 6"):
            assert "_mes" in msg, (name, msg)
        np.testing.assert_array_equal(_bits(abo.MaxValueEntropySearch(ystar)(model, few)), _bits(want))
    # a gradient-enhanced handle
    from tests.test_gpu_gradient_gp import make_grad
    from tests.test_gpu_refine import _grad_problem
    Xg, Yg = _grad_problem(20, 2)
    mg = abo.update(make_grad(O.MATERN52, 0.6, 1.2, 0.05, 3, np.zeros(3)), Xg, Yg)
    zg = np.ascontiguousarray(Xg[:4])
    rc = L.abo_acq_mes(mg._require(), zg.ctypes.data, 4, 2, 0, ys.ctypes.data, len(ys), 0, 0, out.ctypes.data, 0, None, None, 0)
    assert rc == EINVAL and "gradient-enhanced" in abo._lib.last_error()
    rc = L.abo_refine_mes(mg._require(), ys.ctypes.data, len(ys), lo.ctypes.data, up.ctypes.data, 2, zg.ctypes.data, 4, None,
                          xo.ctypes.data, fo.ctypes.data, None)
    assert rc == EINVAL and "gradient-enhanced" in abo._lib.last_error()
    assert L.abo_acq(mg._require(), zg.ctypes.data, 4, 2, 0, 0, 0.01, 0.0, 0, out.ctypes.data, 0, None, None, 0) == 0
    assert np.all(np.isfinite(out))                                                 # the handle still serves what it serves
    with pytest.raises(TypeError):
        abo.evaluate(abo.MaxValueEntropySearch(ystar), mg, zg)
