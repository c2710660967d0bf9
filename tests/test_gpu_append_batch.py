"""GPU tests (-m gpu) of abo_append_batch / append_points: a fitted model conditioned on k more observations in one blocked bordered
step (csrc/append_batch.hip).  The result agrees with the library's refit of all points, with the oracle and with k sequential
appends at the bars every O(N²) update is held to (tests/test_gpu_update.py: _bars, _close_to_refit); the shapes are those at which a
kernel takes another path: one training row, a batch that crosses a 128 / 256 row block, k at, below and above a multiple of 16, the
full 64, several 128-row strips and slices of the block product, and more than 64 points (several steps)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import _lib, synth
from oracle import gp_oracle as O

from tests.test_gpu_parity import FAMS, make_model
from tests.test_gpu_remove import D, ELL, MEAN_C, NOISES, SF2, data, fit, probes
from tests.test_gpu_update import _close_to_refit, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (N0, k): (127, 2) and (120, 16) cross a 128 block, (250, 13) crosses 256, (1500, 17) has twelve strips and every slice of the product
SHAPES = [(1, 2), (5, 3), (120, 16), (127, 2), (128, 64), (129, 33), (250, 13), (300, 64), (1500, 17)]


def n_max_for(N0, k):
    return 2048 if N0 + k > 512 else 512


def state(m, Z):
    """factor and posterior of a model as host arrays (what _same compares)"""
    return abo.get_factor(m) + abo.mean_and_var(m, Z)


def same_state(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def live_views(m):
    out, n = (C.c_int64 * 16)(), C.c_int32(0)
    _lib.check(_lib.lib().abo_test_live_views(m._require(), out, 16, C.byref(n)))
    return list(out[:n.value])


def parity(case, m, family, noise, X, y, seq=None):
    """m against the refit of (X, y), against the oracle and (seq) against the model k sequential appends made"""
    ref = fit(family, noise, X, y)
    st = O.fit(family, ELL, SF2, noise, MEAN_C, X, y)
    _close_to_refit(case, m, ref, probes(), len(y), SF2, noise, st)
    if seq is not None:
        _close_to_refit(case + "_vs_sequential", m, seq, probes(), len(y), SF2, noise)
    Xn, yn = abo.training_data(m)
    np.testing.assert_array_equal(Xn, X)
    np.testing.assert_array_equal(yn, y)


def blocked_and_sequential(family, noise, N0, k):
    X, y = data(N0 + k)
    kw = dict(n_max=n_max_for(N0, k))
    m = abo.append_points(fit(family, noise, X[:N0], y[:N0], **kw), X[N0:], y[N0:])
    assert m.append_path == "appended"
    seq = fit(family, noise, X[:N0], y[:N0], **kw)
    for i in range(N0, N0 + k):
        seq = abo.append(seq, X[i], y[i])
    return m, seq, X, y


def test_one_point_is_append_itself_and_a_set_follows_it():
    N0, noise = 120, 1e-3
    X, y = data(N0 + 1)
    Z = probes()
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512)
    cands = abo.ResidentCandidates(parent, Z)
    a = abo.append_points(parent, X[N0:N0 + 1], y[N0:N0 + 1])
    assert a.append_path == "appended"
    cands.downdate(a)                                           # the view abo_append makes: the set in sync with the parent follows it
    mu_c, var_c = cands.mean_and_var()
    mu_a, var_a = abo.mean_and_var(a, Z)
    np.testing.assert_allclose(mu_c, mu_a, rtol=0, atol=1e-9)
    np.testing.assert_allclose(var_c, var_a, rtol=0, atol=1e-9 * SF2)
    sa = state(a, Z)
    del a, cands                                                # the row goes back: abo_append takes it in place as well
    b = abo.append(parent, X[N0], y[N0])
    same_state(sa, state(b, Z))
    _same(abo.append_points(fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512), X[N0:], y[N0:]), b, Z)


@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("N0,k", SHAPES)
def test_batch_matches_refit_oracle_and_sequential_appends(N0, k, noise):
    m, seq, X, y = blocked_and_sequential(O.MATERN52, noise, N0, k)
    parity(f"append_batch/fam{O.MATERN52}_noise{noise:g}_N{N0}+{k}", m, O.MATERN52, noise, X, y, seq)


@pytest.mark.parametrize("family", sorted(FAMS))
def test_every_family(family):
    N0, k, noise = 129, 33, 1e-3
    m, seq, X, y = blocked_and_sequential(family, noise, N0, k)
    parity(f"append_batch/fam{family}_noise{noise:g}_N{N0}+{k}_families", m, family, noise, X, y, seq)


def test_device_inputs_give_the_same_bits():
    torch = pytest.importorskip("torch")
    N0, k, noise = 129, 33, 1e-3
    X, y = data(N0 + k)
    Z = probes()
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512)
    h = abo.append_points(parent, X[N0:], y[N0:])
    sh = state(h, Z)
    del h
    t = abo.append_points(parent, torch.from_numpy(X[N0:].copy()).cuda(), torch.from_numpy(y[N0:].copy()).cuda())
    assert t.append_path == "appended"
    same_state(sh, state(t, Z))


def test_shared_storage_keeps_every_older_view():
    N0, k, noise = 120, 20, 1e-3
    X, y = data(N0 + 1 + k)
    Z = probes()
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512)
    child = abo.append(parent, X[N0], y[N0])                    # an earlier child: rows 120 are its own
    before = [state(v, Z) for v in (parent, child)]
    grown = abo.append_points(child, X[N0 + 1:], y[N0 + 1:])    # in place, behind the child
    assert grown.append_path == "appended" and live_views(parent) == [N0, N0 + 1, N0 + 1 + k]
    # the parent's sibling view cannot take rows the child holds: it copies on write, and equals update() on the same data bit for bit
    sibling = abo.copy(parent)
    Xo = np.vstack([X[:N0], X[N0 + 5:N0 + 5 + 7]])
    yo = np.concatenate([y[:N0], y[N0 + 5:N0 + 5 + 7]])
    other = abo.append_points(sibling, Xo[N0:], yo[N0:])
    assert other.append_path == "refit"
    _same(other, fit(O.MATERN52, noise, Xo, yo, n_max=512), Z)
    for v, was in zip((parent, child), before):
        same_state(state(v, Z), was)
    parity("append_batch/behind_a_child_N121+20", grown, O.MATERN52, noise, X, y)


def test_full_storage_refits_with_doubled_capacity():
    N0, k, noise = 250, 13, 1e-3                                # n_max = 0: capacity = the fit, 256 rows
    X, y = data(N0 + k + 2)
    m = abo.append_points(fit(O.MATERN52, noise, X[:N0], y[:N0]), X[N0:N0 + k], y[N0:N0 + k])
    assert m.append_path == "refit"
    _same(m, fit(O.MATERN52, noise, X[:N0 + k], y[:N0 + k], n_max=2 * (N0 + k)), probes())
    assert abo.append_points(m, X[N0 + k:], y[N0 + k:]).append_path == "appended"


def test_several_steps_that_will_not_fit_refit_at_once():
    N0, k, noise = 200, 190, 1e-3                               # capacity 384: the first step of 64 would fit, all 190 do not
    X, y = data(N0 + k)
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=300)
    m = abo.append_points(parent, X[N0:], y[N0:])
    assert m.append_path == "refit" and m.timings()["append_trmv_bytes"] == 0.0
    assert live_views(parent) == [N0]
    _same(m, fit(O.MATERN52, noise, X, y, n_max=2 * (N0 + k)), probes())


def test_more_than_64_points_run_in_steps():
    N0, k, noise = 200, 150, 1e-3
    X, y = data(N0 + k)
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512)
    m = abo.append_points(parent, X[N0:], y[N0:])
    assert m.append_path == "appended"
    assert live_views(parent) == [N0, N0 + k]                   # the two intermediate views are gone
    t = m.timings()
    assert t["append_trmv_bytes"] == 8.0 * (200 ** 2 + 264 ** 2 + 328 ** 2)
    parity(f"append_batch/steps_N{N0}+{k}", m, O.MATERN52, noise, X, y)


def test_chained_batches_a_removal_and_another_batch():
    N0, noise = 100, 1e-3
    X, y = data(N0 + 65)
    m = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512)
    for b in range(3):
        lo = N0 + 20 * b
        m = abo.append_points(m, X[lo:lo + 20], y[lo:lo + 20])
        assert m.append_path == "appended"
    m = abo.remove_points(m, 37)
    m = abo.append_points(m, X[N0 + 60:], y[N0 + 60:])
    assert m.append_path == "appended"
    keep = np.setdiff1d(np.arange(N0 + 65), [37])
    parity("append_batch/chained_N100+3x20-1+5", m, O.MATERN52, noise, X[keep], y[keep])


def lattice(n, first=0):
    """n points of a lattice with spacing 7 in D dimensions: under SE with ℓ = 1 their kernel matrix is the identity to 1e-10, so that
    no rounding error decides the sign of a pivot that is zero in exact arithmetic"""
    i = np.arange(first, first + n)
    return np.stack([7.0 * ((i // 3 ** c) % 3) for c in range(D)], axis=1)


def test_failed_batch_reports_the_refit_pivot_and_leaves_the_parent_appendable():
    N0 = 5
    X = lattice(N0 + 12)
    y = np.linspace(-1.0, 1.0, N0 + 12)
    Z = lattice(8, 40) + 0.5
    mk = lambda **kw: make_model(O.SE, 1.0, 1.0, 0.0, n_max=64, **kw)
    parent = abo.update(mk(), X[:N0], y[:N0])
    was = state(parent, Z)
    Xb = X[N0:N0 + 6].copy()
    Xb[3] = Xb[1]                                               # row 3 repeats row 1
    with pytest.raises(abo.PosDefException) as e_ref:
        abo.update(mk(), np.vstack([X[:N0], Xb]), y[:N0 + 6])
    with pytest.raises(abo.PosDefException) as e:
        abo.append_points(parent, Xb, y[N0:N0 + 6])
    assert e.value.info == e_ref.value.info == N0 + 4
    assert live_views(parent) == [N0]                           # the claimed rows are given back
    Xt = X[N0:N0 + 3].copy()
    Xt[0] = X[2]                                                # the first row repeats a training point
    with pytest.raises(abo.PosDefException) as e:
        abo.append_points(parent, Xt, y[N0:N0 + 3])
    assert e.value.info == N0 + 1
    same_state(state(parent, Z), was)
    ok = abo.append_points(parent, X[N0 + 6:], y[N0 + 6:])
    assert ok.append_path == "appended"
    assert np.max(np.abs(abo.posterior_mean(ok, X[N0 + 6:]) - y[N0 + 6:])) < 1e-9


def test_refusals_name_the_call():
    L = _lib.lib()
    N0 = 30
    X, y = data(N0 + 2)
    src = fit(O.MATERN52, 1e-3, X[:N0], y[:N0], n_max=64)
    xb, yb = np.ascontiguousarray(X[N0:]), np.ascontiguousarray(y[N0:])
    out, info = C.c_void_p(), C.c_int64(0)

    def call(h, xp, k, d, yp):
        return L.abo_append_batch(h, xp, k, d, yp, _lib.HOST, C.byref(info), C.byref(out))

    for args, text in (((None, xb.ctypes.data, 2, D, yb.ctypes.data), "null"), ((src._require(), None, 2, D, yb.ctypes.data), "null"),
                       ((src._require(), xb.ctypes.data, 2, D, None), "null"), ((src._require(), xb.ctypes.data, 0, D, yb.ctypes.data), "k = 0"),
                       ((src._require(), xb.ctypes.data, -1, D, yb.ctypes.data), "k = -1"),
                       ((src._require(), xb.ctypes.data, 2, D + 1, yb.ctypes.data), "dimension")):
        assert call(*args) == _lib.ABO_EINVAL, text
        assert text in _lib.last_error() and "abo_append_batch" in _lib.last_error()
    hp = C.c_void_p()
    prm = src._params()
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    assert call(hp, xb.ctypes.data, 2, D, yb.ctypes.data) == _lib.ABO_EINVAL
    assert "not conditioned" in _lib.last_error() and "abo_append_batch" in _lib.last_error()
    _lib.check(L.abo_destroy(hp))
    Xg = synth.points(14, 6, 2)
    Yg = np.column_stack([synth.objective(Xg, 0.05), np.zeros((6, 2))])
    grad = abo.update(abo.HipGradientGP(abo.Matern52Kernel(), 3, 1e-3), Xg, Yg)
    assert call(grad._require(), xb.ctypes.data, 2, 2, yb.ctypes.data) == _lib.ABO_EINVAL
    assert "gradient-enhanced" in _lib.last_error() and "abo_append_batch" in _lib.last_error()
    assert out.value is None
    with pytest.raises(_lib.DimensionMismatch, match="dimension"):
        abo.append_points(src, np.zeros((2, D + 1)), yb)
    assert live_views(src) == [N0]
    assert abo.append_points(src, xb, yb).append_path == "appended"


def test_the_result_counts_as_an_appended_view():
    N0, k, noise = 129, 33, 1e-2
    X, y = data(N0 + k + 1)
    Z = probes()
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512)
    cands = abo.ResidentCandidates(parent, Z)
    m = abo.append_points(parent, X[N0:N0 + k], y[N0:N0 + k])
    with pytest.raises(ValueError, match="abo_cand_refresh"):   # k ≥ 2: the set stays with the parent
        cands.downdate(m)
    L = _lib.lib()
    o = [C.c_double(float("nan")) for _ in range(3)]
    assert L.abo_nlml_grad(m._require(), *(C.byref(x) for x in o)) == _lib.ABO_EINVAL
    cands.refresh(m)
    ref = fit(O.MATERN52, noise, X[:N0 + k], y[:N0 + k])
    mu, var = cands.mean_and_var()
    mu_r, var_r = abo.mean_and_var(ref, Z)
    assert np.max(np.abs(mu - mu_r)) < 1e-9 and np.max(np.abs(var - var_r)) < 1e-9 * SF2
    for name, a, b in zip(("mu", "var", "lpd", "nlpl"), abo.leave_one_out(m), abo.leave_one_out(ref)):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) < 1e-9, name
    assert np.max(np.abs(abo.posterior_cov(m, Z[:64]) - abo.posterior_cov(ref, Z[:64]))) < 1e-9 * SF2
    Zb = synth.points(13, 4096, D)
    acq = abo.ExpectedImprovement(0.01, float(np.min(y[:N0 + k])))
    for contraction in ("fp64", "int8"):
        mc = abo.append_points(fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512, contraction=contraction), X[N0:N0 + k], y[N0:N0 + k])
        rc = fit(O.MATERN52, noise, X[:N0 + k], y[:N0 + k], contraction=contraction)
        s, tv, ti = abo.evaluate(acq, mc, Zb, k=16)
        sr, tvr, tir = abo.evaluate(acq, rc, Zb, k=16)
        assert mc.timings()["contraction_engine"] == rc.timings()["contraction_engine"]
        np.testing.assert_array_equal(ti, tir)
        assert np.max(np.abs(s - sr)) < 1e-9 * max(1.0, np.max(np.abs(sr)))
    # it grows and shrinks again: append, append_points, remove_points and update (as prev)
    g = abo.append(m, X[N0 + k], y[N0 + k])
    assert abo.training_data(g)[0].shape[0] == N0 + k + 1
    assert abo.training_data(abo.remove_points(m, 3))[0].shape[0] == N0 + k - 1
    del g
    inc = abo.append_points(fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512, incremental_update=True), X[N0:N0 + k], y[N0:N0 + k])
    assert abo.update(inc, X, y).update_path == "appended"


@pytest.mark.parametrize("N0,k", [(300, 64), (1500, 17)])
def test_two_calls_give_the_same_bits(N0, k):
    X, y = data(N0 + k)
    Z = probes()
    parent = fit(O.MATERN52, 1e-3, X[:N0], y[:N0], n_max=n_max_for(N0, k))
    first = abo.append_points(parent, X[N0:], y[N0:])
    s1 = state(first, Z)
    del first                                                   # destroyed before the second call: both run in place, on the same rows
    second = abo.append_points(parent, X[N0:], y[N0:])
    assert second.append_path == "appended"
    same_state(s1, state(second, Z))


@pytest.mark.parametrize("lower", [1, 0])
@pytest.mark.parametrize("k", [1, 16, 17, 64])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 1500])
def test_the_skinny_triangular_product_alone(N, k, lower):
    """abo_test_tri_skinny against NumPy on a FULL random matrix (the triangle is the kernel's to cut out) in a storage image with NaN
    in every row and column ≥ N.  Bar: the forward bound of a length-N dot product at twice the unit round-off per term."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(1000 * N + 10 * k + lower)
    cap = (N + 127) // 128 * 128 + 128
    kp = (k + 15) // 16 * 16
    W = rng.standard_normal((N, N))
    V = np.zeros((N, kp))
    V[:, :k] = rng.standard_normal((N, k))
    img = np.full((cap, cap), np.nan)
    img[:N, :N] = W
    Wd, Vd = torch.from_numpy(img).cuda(), torch.from_numpy(V).cuda()
    out = torch.full((N, kp), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().abo_test_tri_skinny(0, Wd.data_ptr(), cap, Vd.data_ptr(), out.data_ptr(), N, k, lower))
    ref = (np.tril(W) if lower else np.triu(W)) @ V
    got = out.cpu().numpy()
    err = np.max(np.abs(got - ref))
    bar = 4e-16 * N * np.max(np.abs(W)) * np.max(np.abs(V))
    print(f"tri_skinny N={N} k={k} lower={lower}: err {err:.3e} bar {bar:.3e}")
    assert np.all(np.isfinite(got)) and err <= bar
    assert np.all(got[:, k:] == 0.0)


def test_timings_count_one_stream_of_each_triangle():
    """With ABO_PHASE_EVENTS=1 (read once per process, so: a child process) the new handle reports the device time of the two block
    products and 8·N² bytes for the one blocked step — at N₀ = 100, one 128-row block, where the automatic mode would record no events."""
    code = ("import json, numpy as np, abstractbayesopt.jl_amd as abo\n"
            "from tests.test_gpu_remove import data, fit\n"
            "from oracle import gp_oracle as O\n"
            "X, y = data(110)\n"
            "m = abo.append_points(fit(O.MATERN52, 1e-3, X[:100], y[:100], n_max=128), X[100:], y[100:])\n"
            "t = m.timings()\n"
            "print('TIMINGS ' + json.dumps({'path': m.append_path, 'ms': t['append_trmv_ms'], 'bytes': t['append_trmv_bytes']}))\n")
    env = dict(os.environ, ABO_PHASE_EVENTS="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    t = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TIMINGS ")][0][8:])
    assert t["path"] == "appended"
    assert t["bytes"] == 8.0 * 100 * 100                        # one stream of each triangle, not k
    assert t["ms"] > 0.0


def test_a_set_last_synced_one_row_below_a_batch_view_is_refused():
    """The set followed a one-point child of the parent (N + 1 rows) that is gone; a batch of two from the parent then has N + 2 rows
    on the same storage, one more than the set was synced with — and still is no one-point append: ABO_EINVAL, before any device work."""
    N0, noise = 120, 1e-3
    X, y = data(N0 + 2)
    Z = probes()
    parent = fit(O.MATERN52, noise, X[:N0], y[:N0], n_max=512)
    cands = abo.ResidentCandidates(parent, Z)
    a = abo.append(parent, X[N0], y[N0])
    cands.downdate(a)
    mu0, var0 = cands.mean_and_var()
    cands.model = parent                                        # (the Python object keeps no reference to `a`)
    del a
    m = abo.append_points(parent, X[N0:], y[N0:])
    assert m.append_path == "appended" and live_views(parent) == [N0, N0 + 2]
    assert _lib.lib().abo_cand_downdate(m._require(), cands._h.ptr) == _lib.ABO_EINVAL
    assert "abo_cand_downdate" in _lib.last_error() and "abo_cand_refresh" in _lib.last_error()
    with pytest.raises(ValueError, match="abo_cand_refresh"):
        cands.downdate(m)
    cands.refresh(m)
    mu, var = cands.mean_and_var()
    mu_m, var_m = abo.mean_and_var(m, Z)
    np.testing.assert_allclose(mu, mu_m, rtol=0, atol=1e-9)
    np.testing.assert_allclose(var, var_m, rtol=0, atol=1e-9 * SF2)
    assert np.max(np.abs(mu - mu0)) > 0.0                       # (the refresh did change the stored posterior)
