"""GPU tests (-m gpu) of abo_remove / remove_points: a fitted model without some of its observations in O(N²) (csrc/remove.hip).
The result agrees with a refit of the remaining data at the bars an O(N²) update is held to against a refit (tests/test_gpu_update.py:
_bars, _close_to_refit) and with the NumPy oracle; the shapes are those at which the kernels take another path: one row, the padded
size changing at 128 and 256, rows before / at / behind j, a row that spans several 256-element scan steps with j at a step's edge."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import _lib, synth
from oracle import gp_oracle as O

from tests.parity_record import check
from tests.test_gpu_parity import FAMS, make_model
from tests.test_gpu_update import _bars, _close_to_refit, _same

D, ELL, SF2, MEAN_C = 4, 0.8, 1.3, 0.5
NOISES = (1e-3, 1e-2)
STEP = 256                                   # REMOVE_SCAN_CHUNK: elements of a row per scan step
BIG = 1500                                   # rows of up to six scan steps
# (N, j): j = 0 is the longest scan, j = N − 1 none at all; BIG: m = N − 1 − j trailing rows at a step's edge ± 1, and j itself there
SHAPES = [(129, 0), (129, 127), (129, 128), (130, 64), (257, 0), (257, 255), (257, 256)] + \
         [(BIG, j) for j in (0, STEP - 1, STEP, STEP + 1, BIG - 1 - STEP - 1, BIG - 1 - STEP, BIG - 1 - STEP + 1, BIG - 1)]


@lru_cache(maxsize=None)
def data(N, seed=11):
    X = synth.points(seed, N, D)
    y = synth.objective(X, 0.05) + MEAN_C
    X.setflags(write=False); y.setflags(write=False)
    return X, y


@lru_cache(maxsize=None)
def probes(M=300):
    Z = synth.points(12, M, D)
    Z.setflags(write=False)
    return Z


def fit(family, noise, X, y, **kw):
    return abo.update(make_model(family, ELL, SF2, noise, MEAN_C, **kw), X, y)


@lru_cache(maxsize=None)
def source(family, noise, N):
    X, y = data(N)
    return fit(family, noise, X, y)


def parity(case, m, family, noise, X, y):
    """m against the refit of (X, y) and against the oracle, every metric of _close_to_refit"""
    ref = fit(family, noise, X, y)
    st = O.fit(family, ELL, SF2, noise, MEAN_C, X, y)
    _close_to_refit(case, m, ref, probes(), len(y), SF2, noise, st)
    Xn, yn = abo.training_data(m)
    np.testing.assert_array_equal(Xn, X)
    np.testing.assert_array_equal(yn, y)
    return ref


def keep_of(N, idx):
    return np.setdiff1d(np.arange(N), np.atleast_1d(idx))


@pytest.mark.parametrize("family", sorted(FAMS))
@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("j", [0, 1])
def test_two_points_every_family(family, noise, j):
    X, y = data(2)
    m = abo.remove_points(source(family, noise, 2), j)
    assert m.remove_path == "removed"
    k = keep_of(2, j)
    parity(f"remove/fam{family}_noise{noise:g}_N2_j{j}", m, family, noise, X[k], y[k])


@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("N,j", SHAPES)
def test_one_removal_matches_refit_and_oracle(N, j, noise):
    X, y = data(N)
    m = abo.remove_points(source(O.MATERN52, noise, N), j)
    assert m.remove_path == "removed"
    k = keep_of(N, j)
    parity(f"remove/fam{O.MATERN52}_noise{noise:g}_N{N}_j{j}", m, O.MATERN52, noise, X[k], y[k])


def test_several_indices_run_as_removals():
    N, noise = 300, 1e-3
    X, y = data(N)
    idx = [N - 1, 0, 128, 64]                                   # any order
    m = abo.remove_points(source(O.MATERN52, noise, N), idx)
    assert m.remove_path == "removed"
    k = keep_of(N, idx)
    parity(f"remove/k4_N{N}", m, O.MATERN52, noise, X[k], y[k])


def test_beyond_the_rule_refits_bit_for_bit():
    N, noise = 300, 1e-3
    X, y = data(N)
    idx = np.arange(3, 3 + 2 * 5, 2)                            # kmax(300) = 4: five indices refit
    m = abo.remove_points(source(O.MATERN52, noise, N), idx)
    assert m.remove_path == "refit"
    k = keep_of(N, idx)
    _same(m, fit(O.MATERN52, noise, X[k], y[k]), probes())


def test_appended_views_and_a_parent_with_a_live_child():
    N0, add, noise = 120, 10, 1e-3
    X, y = data(N0 + add)
    Z = probes()
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=256)
    child = parent
    for i in range(N0, N0 + add):
        child = abo.append(child, X[i], y[i])
    before = [abo.get_factor(v) + abo.mean_and_var(v, Z) for v in (parent, child)]
    a = abo.remove_points(child, 60)                            # from the appended view
    b = abo.remove_points(parent, 119)                          # from the parent while the child lives: rows ≥ 120 are the child's
    c = abo.remove_points(parent, 0)
    for v, was in zip((parent, child), before):
        for u, w in zip(abo.get_factor(v) + abo.mean_and_var(v, Z), was):
            np.testing.assert_array_equal(u, w)
    k = keep_of(N0 + add, 60)
    parity("remove/appended_view_N130_j60", a, O.MATERN52, noise, X[k], y[k])
    parity("remove/parent_N120_j119", b, O.MATERN52, noise, X[:N0 - 1], y[:N0 - 1])
    parity("remove/parent_N120_j0", c, O.MATERN52, noise, X[1:N0], y[1:N0])


def test_sliding_window():
    N, steps, noise = 200, 30, 1e-3
    X, y = data(N + steps)
    m = fit(O.MATERN52, noise, X[:N], y[:N], n_max=256)
    for i in range(steps):
        m = abo.remove_points(m, 0)
        assert m.remove_path == "removed"
        m = abo.append(m, X[N + i], y[N + i])
    # the drift of 30 removals and 30 appends is what the record keeps: the same metrics, the same bars
    parity(f"remove/window_N{N}_steps{steps}", m, O.MATERN52, noise, X[steps:], y[steps:])


def test_removed_model_predicts_the_leave_one_out_values():
    N, noise = 300, 1e-2
    X, y = data(N)
    src = source(O.MATERN52, noise, N)
    mu_l, var_l, _, _ = abo.leave_one_out(src)
    _, post = _bars(N, SF2, noise)
    for j in (0, N // 2, N - 1):
        mu, var = abo.mean_and_var(abo.remove_points(src, j), X[j:j + 1])
        check(f"remove/loo_N{N}_j{j}", "mu", abs(mu[0] - mu_l[j]) / max(1.0, abs(mu_l[j])), post)
        check(f"remove/loo_N{N}_j{j}", "var", abs(var[0] + noise - var_l[j]) / SF2, post)


@lru_cache(maxsize=None)
def downstream(contraction=None):
    """a removed model and the refit of its data, for the entry points that follow"""
    N, noise, j = 300, 1e-2, 77
    X, y = data(N)
    k = keep_of(N, j)
    kw = {} if contraction is None else {"contraction": contraction}
    return abo.remove_points(fit(O.MATERN52, noise, X, y, **kw), j), fit(O.MATERN52, noise, X[k], y[k], **kw), _bars(N, SF2, noise)[1]


def test_downstream_nlml_gradients():
    m, ref, post = downstream()
    L = _lib.lib()
    out = []
    for g in (m, ref):
        o = [C.c_double(float("nan")) for _ in range(3)]
        _lib.check(L.abo_nlml_grad(g._require(), *(C.byref(x) for x in o)))
        a = [C.c_double(float("nan")) for _ in range(3)]
        ell = (C.c_double * D)()
        _lib.check(L.abo_nlml_grad_ard(g._require(), D, C.byref(a[0]), ell, C.byref(a[1]), C.byref(a[2])))
        out.append(np.array([x.value for x in o] + [a[0].value] + list(ell) + [a[1].value, a[2].value]))
    scale = max(1.0, np.max(np.abs(out[1])))
    assert np.all(np.isfinite(out[0]))
    check("remove/downstream_N300", "nlml_grad", np.max(np.abs(out[0] - out[1])) / scale, post)


def test_downstream_leave_one_out_and_covariance():
    m, ref, post = downstream()
    for name, a, b in zip(("loo_mu", "loo_var", "loo_lpd", "loo_nlpl"), abo.leave_one_out(m), abo.leave_one_out(ref)):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        check("remove/downstream_N300", name, np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))), min(post, 1e-9))
    Z = probes()[:64]
    check("remove/downstream_N300", "cov", np.max(np.abs(abo.posterior_cov(m, Z) - abo.posterior_cov(ref, Z))) / SF2, post)


@pytest.mark.parametrize("contraction", ["fp64", "int8"])
def test_downstream_topk_under_both_engines(contraction):
    m, ref, post = downstream(contraction)
    Z = synth.points(13, 4096, D)
    acq = abo.ExpectedImprovement(0.01, float(np.min(abo.training_data(ref)[1])))
    s, tv, ti = abo.evaluate(acq, m, Z, k=16)
    sr, tvr, tir = abo.evaluate(acq, ref, Z, k=16)
    assert m.timings()["contraction_engine"] == ref.timings()["contraction_engine"]
    np.testing.assert_array_equal(ti, tir)
    scale = max(1.0, np.max(np.abs(sr)))
    check(f"remove/downstream_N300_{contraction}", "ei", np.max(np.abs(s - sr)) / scale, post)
    check(f"remove/downstream_N300_{contraction}", "ei_top", np.max(np.abs(tv - tvr)) / scale, post)


def test_downstream_optimizer_resident_set_and_paths():
    m, ref, post = downstream()
    X, y = abo.training_data(ref)
    acq = abo.ExpectedImprovement(0.01, float(np.min(y)))
    dom = abo.ContinuousDomain(np.zeros(D), np.ones(D))
    best = [abo.optimize_acquisition(acq, g, dom, n_grid=2000, n_local=8, rng=np.random.default_rng(5)) for g in (m, ref)]
    f = abo.evaluate(acq, ref, np.stack(best))[0]
    check("remove/downstream_N300", "optimize_value", abs(f[0] - f[1]) / max(1.0, abs(f[1])), 1e-6)
    Z = probes()
    cands = abo.ResidentCandidates(source(O.MATERN52, 1e-2, 300), Z)      # in sync with the model before the removal
    cands.refresh(m)
    mu, var = cands.mean_and_var()
    mu_r, var_r = abo.mean_and_var(ref, Z)
    check("remove/downstream_N300", "set_mu", np.max(np.abs(mu - mu_r)) / max(1.0, np.max(np.abs(mu_r))), post)
    check("remove/downstream_N300", "set_var", np.max(np.abs(var - var_r)) / SF2, post)
    pa, pb = (abo.sample_paths(g, 8, R=256, rng=7)(Z) for g in (m, ref))
    check("remove/downstream_N300", "paths", np.max(np.abs(pa - pb)) / max(1.0, np.max(np.abs(pb))), post * 10)
    # and it grows again: append and update (as prev) take it as a freshly fitted model
    Xs, ys = data(301)
    grown = abo.append(m, Xs[300], ys[300])
    assert abo.training_data(grown)[0].shape[0] == 300
    inc = abo.remove_points(fit(O.MATERN52, 1e-2, *data(300), n_max=512, incremental_update=True), 77)
    up = abo.update(inc, np.vstack([X, Xs[300:]]), np.append(y, ys[300]))
    assert up.update_path == "appended"


def test_two_calls_give_the_same_bits():
    src = source(O.MATERN52, 1e-3, 257)
    for idx in (0, [5, 200]):
        _same(abo.remove_points(src, idx), abo.remove_points(src, idx), probes())


def test_error_paths_leave_the_model_usable():
    L = _lib.lib()
    src = source(O.MATERN52, 1e-3, 130)
    out, path = C.c_void_p(), C.c_int32(-1)

    def call(h, idx):
        a = np.asarray(idx, dtype=np.int64)
        return L.abo_remove(h, a.ctypes.data, len(a), C.byref(path), C.byref(out))

    for bad, text in (([130], "outside"), ([-1], "outside"), ([5, 5], "increasing"), ([7, 3], "increasing"),
                      (list(range(130)), "leaves none")):
        assert call(src._require(), bad) == _lib.ABO_EINVAL, bad
        assert text in _lib.last_error() and "abo_remove" in _lib.last_error()
    with pytest.raises(ValueError, match="outside"):
        abo.remove_points(src, 130)
    hp = C.c_void_p()
    prm = src._params()
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    assert call(hp, [0]) == _lib.ABO_EINVAL and "not conditioned" in _lib.last_error()
    _lib.check(L.abo_destroy(hp))
    Xg = synth.points(14, 6, 2)
    Yg = np.column_stack([synth.objective(Xg, 0.05), np.zeros((6, 2))])
    grad = abo.update(abo.HipGradientGP(abo.Matern52Kernel(), 3, 1e-3), Xg, Yg)
    assert call(grad._require(), [0]) == _lib.ABO_EINVAL and "gradient-enhanced" in _lib.last_error()
    assert out.value is None
    X, y = data(130)
    parity("remove/after_errors_N130_j129", abo.remove_points(src, 129), O.MATERN52, 1e-3, X[:129], y[:129])


def test_ard_model_predicts_like_the_ard_refit():
    N, noise, j = 130, 1e-3, 64
    X, y = data(N)
    ells = (0.5, 0.8, 1.1, 2.0)
    mk = lambda: abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), ells), noise, mean=abo.ConstMean(MEAN_C))
    m = abo.remove_points(abo.update(mk(), X, y), j)
    k = keep_of(N, j)
    ref = abo.update(mk(), X[k], y[k])
    assert abo.ard_lengthscales(m) is not None
    _close_to_refit(f"remove/ard_N{N}_j{j}", m, ref, probes(), N - 1, SF2, noise)
    np.testing.assert_allclose(abo.training_data(m)[0], X[k], rtol=4e-16, atol=0)
