"""GPU tests (-m gpu) of abo_update / abo_mgpu_update: update(model, xs, ys) on a model built with incremental_update=True, as
the reference's BO loop calls it every iteration (src/bayesian_opt.jl:119-125).  When (xs, ys) extends the model's data the
result comes from bordered appends and agrees with the refit to rounding (the append/* bars of test_gpu_incremental.py);
every other case is the refit itself, bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

from tests.parity_record import check
from tests.test_gpu_parity import FAMS, make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bars(N, sf2, noise):
    tol = max(1e-11, 4e-16 * (1 + N * sf2 / noise))
    return tol, min(1e-6, tol * 1e2)


def _same(a, b, Z):
    """two models whose posterior and factor agree bit for bit"""
    mu_a, var_a = abo.mean_and_var(a, Z)
    mu_b, var_b = abo.mean_and_var(b, Z)
    np.testing.assert_array_equal(mu_a, mu_b)
    np.testing.assert_array_equal(var_a, var_b)
    for u, v in zip(abo.get_factor(a), abo.get_factor(b)):
        np.testing.assert_array_equal(u, v)


def _close_to_refit(case, m, ref, Z, N, sf2, noise, st=None):
    tol, post = _bars(N, sf2, noise)
    L, al, Li = abo.get_factor(m)
    Lr, alr, _ = abo.get_factor(ref)
    check(case, "L_vs_own_refit", np.max(np.abs(L - Lr)), tol * 2)
    check(case, "LinvL_minus_I", np.max(np.abs(Li @ Lr - np.eye(N))), tol * 20)
    mu, var = abo.mean_and_var(m, Z)
    mu_r, var_r = abo.mean_and_var(ref, Z)
    check(case, "mu_vs_own_refit", np.max(np.abs(mu - mu_r)) / max(1.0, np.max(np.abs(mu_r))), post)
    check(case, "var_vs_own_refit", np.max(np.abs(var - var_r)) / sf2, post)
    if st is not None:
        check(case, "L", np.max(np.abs(L - st.L)), tol * 2)
        check(case, "alpha_rel", np.max(np.abs(al - st.alpha)) / max(1.0, np.max(np.abs(st.alpha))), min(1e-6, tol * 1e3))
        mu_o, var_o = O.predict(st, Z)
        check(case, "mu", np.max(np.abs(mu - mu_o)) / max(1.0, np.max(np.abs(mu_o))), post)
        check(case, "var", np.max(np.abs(var - var_o)) / sf2, post)
        check(case, "nlml_rel", abs(abo.nlml_fitted(m) - O.nlml(st)) / max(1.0, abs(O.nlml(st))), post)


def test_driver_shaped_loop_appends_and_matches_refit_and_oracle():
    d, N0, iters, ell, sf2, noise, mean_c = 4, 120, 20, 1.0, 1.3, 1e-3, 0.5
    X = synth.points(1, N0 + iters, d)
    y = synth.objective(X, 0.05) + mean_c
    Z = synth.points(2, 777, d)
    m = abo.update(make_model(O.MATERN52, ell, sf2, noise, mean_c, n_max=256, incremental_update=True), X[:N0], y[:N0])
    assert m.update_path == "refit" and m.incremental_update
    for j in range(1, iters + 1):
        m = abo.update(m, X[:N0 + j], y[:N0 + j])
        assert m.update_path == "appended", j
    N = N0 + iters
    ref = abo.update(make_model(O.MATERN52, ell, sf2, noise, mean_c), X, y)
    st = O.fit(O.MATERN52, ell, sf2, noise, mean_c, X, y)
    _close_to_refit(f"update/loop_fam{O.MATERN52}_d{d}_N{N0}+{iters}", m, ref, Z, N, sf2, noise, st)


def test_c3_shape_appends_match_refit():
    d, N, iters, ell, sf2, noise = 8, 8192, 4, 1.0, 1.0, 1e-2
    X = synth.points(3, N, d)
    y = synth.objective(X, 0.05)
    Z = synth.points(4, 65536, d)
    N0 = N - iters
    m = abo.update(make_model(O.MATERN52, ell, sf2, noise, n_max=N + 128, incremental_update=True), X[:N0], y[:N0])
    for j in range(1, iters + 1):
        m = abo.update(m, X[:N0 + j], y[:N0 + j])
        assert m.update_path == "appended"
    ref = abo.update(make_model(O.MATERN52, ell, sf2, noise), X, y)
    tol, post = _bars(N, sf2, noise)
    mu, var = abo.mean_and_var(m, Z)
    mu_r, var_r = abo.mean_and_var(ref, Z)
    case = f"update/c3_fam{O.MATERN52}_d{d}_N{N0}+{iters}"
    check(case, "mu_vs_own_refit", np.max(np.abs(mu - mu_r)) / max(1.0, np.max(np.abs(mu_r))), post)
    check(case, "var_vs_own_refit", np.max(np.abs(var - var_r)) / sf2, post)
    check(case, "nlml_rel_vs_own_refit", abs(abo.nlml_fitted(m) - abo.nlml_fitted(ref)) / max(1.0, abs(abo.nlml_fitted(ref))), post)


def _base(n_max=512, N0=200, d=3, noise=1e-3, jitter=0.0):
    X = synth.points(5, N0 + 120, d)
    y = synth.objective(X, 0.05)
    mk = lambda **kw: make_model(O.MATERN52, 0.8, 1.3, noise, n_max=n_max, jitter=jitter, **kw)
    return X, y, mk, abo.update(mk(incremental_update=True), X[:N0], y[:N0])


def test_falls_back_to_the_refit_bit_for_bit():
    N0 = 200
    X, y, mk, m = _base()
    Z = synth.points(6, 300, 3)

    def refit_case(Xn, yn, model=None, plain=None):
        out = abo.update(model or m, Xn, yn)
        assert out.update_path == "refit"
        _same(out, abo.update(plain or mk(), Xn, yn), Z)

    Xu = X[:N0 + 1].copy()
    Xu[5, 1] = np.nextafter(Xu[5, 1], np.inf)                      # one prefix coordinate, one ulp
    refit_case(Xu, y[:N0 + 1])
    yu = y[:N0 + 1].copy()
    yu[7] += 1e-3                                                   # one prefix target
    refit_case(X[:N0 + 1], yu)
    mu0, _ = abo.get_mean_std(m, y[:N0 + 1], "mean_only")          # re-centred targets (the C1 loop's mean_only standardisation)
    refit_case(X[:N0 + 1], abo.std_y(m, y[:N0 + 1], mu0, 1.0))
    other = abo.copy(m)                                             # other hyper-parameters on prev's handle
    other.kernel = 1.3 * abo.with_lengthscale(abo.Matern52Kernel(), 0.9)
    plain = make_model(O.MATERN52, 0.9, 1.3, 1e-3, n_max=512)
    refit_case(X[:N0 + 1], y[:N0 + 1], model=other, plain=plain)
    refit_case(X[:N0 - 3], y[:N0 - 3])                              # N < Nprev
    refit_case(X[:N0 + 100], y[:N0 + 100])                          # k beyond the crossover rule (at most 64 rows)
    # the model is still appendable after all of that
    assert abo.update(m, X[:N0 + 1], y[:N0 + 1]).update_path == "appended"


def test_jittered_prev_goes_back_through_the_refit():
    X = np.array([[0.1, 0.2], [0.1, 0.2], [0.7, 0.3], [0.4, 0.9]])
    y = np.array([0.5, 0.5, -0.2, 0.8])
    Z = synth.points(6, 50, 2)
    mk = lambda **kw: make_model(O.SE, 0.5, 1.0, 0.0, n_max=64, jitter=1e-8, **kw)
    m = abo.update(mk(incremental_update=True), X[:3], y[:3])       # duplicate point, zero noise: the jitter ladder ran
    out = abo.update(m, X, y)
    assert out.update_path == "refit"
    _same(out, abo.update(mk(), X, y), Z)


def test_full_storage_refits_with_doubled_capacity_then_appends():
    N0 = 256                                                       # n_max = 0: capacity = the fit, 256 points (two row blocks)
    X, y, mk, m = _base(n_max=0, N0=N0)
    Z = synth.points(6, 300, 3)
    out = abo.update(m, X[:N0 + 1], y[:N0 + 1])
    assert out.update_path == "refit"
    _same(out, abo.update(make_model(O.MATERN52, 0.8, 1.3, 1e-3, n_max=2 * (N0 + 1)), X[:N0 + 1], y[:N0 + 1]), Z)
    nxt = abo.update(out, X[:N0 + 2], y[:N0 + 2])
    assert nxt.update_path == "appended"
    _close_to_refit("update/grow_N256+2", nxt, abo.update(mk(), X[:N0 + 2], y[:N0 + 2]), Z, N0 + 2, 1.3, 1e-3)


def test_same_data_shares_prev():
    N0 = 200
    X, y, mk, m = _base()
    Z = synth.points(6, 300, 3)
    out = abo.update(m, X[:N0], y[:N0])
    assert out.update_path == "shared"
    _same(out, m, Z)


def test_failed_append_raises_like_the_refit_and_leaves_prev_appendable():
    # test/test_bayesian_opt.jl:749-786: zero noise, then a point 1e-12 from an existing one
    X = np.array([[-1.0, -1.0], [5.0, -5.0]])
    y = np.array([1.0, 2.0])
    Z = np.array([[0.0, 0.0], [2.0, 1.0], [-1.0, -0.5]])
    mk = lambda **kw: make_model(O.SE, 1.0, 1.0, 0.0, n_max=16, **kw)
    m = abo.update(mk(incremental_update=True), X, y)
    mu0, var0 = abo.mean_and_var(m, Z)
    Xb = np.vstack([X, [[-1.0 + 1e-12, -1.0 + 1e-12]]])
    yb = np.append(y, 1.0)
    with pytest.raises(abo.PosDefException) as e_ref:
        abo.update(mk(), Xb, yb)
    with pytest.raises(abo.PosDefException) as e:
        abo.update(m, Xb, yb)
    assert e.value.info == e_ref.value.info == 3
    mu1, var1 = abo.mean_and_var(m, Z)
    np.testing.assert_array_equal(mu0, mu1)
    np.testing.assert_array_equal(var0, var1)
    ok = abo.update(m, np.vstack([X, [[2.0, 2.0]]]), np.append(y, 0.5))
    assert ok.update_path == "appended"
    assert abs(abo.posterior_mean(ok, [[2.0, 2.0]])[0] - 0.5) < 1e-9
    # with jitter > 0 the same inputs take the refit's jitter ladder, exactly as abo_fit
    mj = lambda **kw: make_model(O.SE, 1.0, 1.0, 0.0, n_max=16, jitter=1e-6, **kw)
    pj = abo.update(mj(incremental_update=True), X, y)
    out = abo.update(pj, Xb, yb)
    assert out.update_path == "refit"
    _same(out, abo.update(mj(), Xb, yb), Z)


def test_rollback_and_diverging_updates():
    N0 = 200
    X, y, mk, m = _base()
    Z = synth.points(6, 300, 3)
    prev = abo.copy(m)
    mu0, var0 = abo.mean_and_var(prev, Z)
    m1 = abo.update(m, X[:N0 + 1], y[:N0 + 1])
    assert m1.update_path == "appended"
    mu1, var1 = abo.mean_and_var(prev, Z)
    np.testing.assert_array_equal(mu0, mu1)
    np.testing.assert_array_equal(var0, var1)
    # a second child of the same parent with another new point: the rows past prev are taken, so it copies on write
    Xo = np.vstack([X[:N0], X[N0 + 5:N0 + 6]])
    yo = np.append(y[:N0], y[N0 + 5])
    m2 = abo.update(prev, Xo, yo)
    assert m2.update_path == "refit"
    _close_to_refit("update/diverge_a", m1, abo.update(mk(), X[:N0 + 1], y[:N0 + 1]), Z, N0 + 1, 1.3, 1e-3)
    _same(m2, abo.update(mk(), Xo, yo), Z)


def test_device_inputs_take_the_same_path():
    torch = pytest.importorskip("torch")
    N0 = 200
    X, y, mk, m = _base()
    Z = synth.points(6, 300, 3)
    h = abo.update(m, X[:N0 + 2], y[:N0 + 2])
    assert h.update_path == "appended"
    mu_h, var_h = abo.mean_and_var(h, Z)
    f_h = abo.get_factor(h)
    del h                                                          # its rows go back: the device-input update appends in place too
    Xt = torch.from_numpy(np.ascontiguousarray(X[:N0 + 2])).cuda()
    yt = torch.from_numpy(np.ascontiguousarray(y[:N0 + 2])).cuda()
    t = abo.update(m, Xt, yt)
    assert t.update_path == "appended"
    mu_t, var_t = abo.mean_and_var(t, Z)
    np.testing.assert_array_equal(mu_h, mu_t)
    np.testing.assert_array_equal(var_h, var_t)
    for u, v in zip(f_h, abo.get_factor(t)):
        np.testing.assert_array_equal(u, v)
    # a device prefix that differs falls back as well
    Xt2 = Xt.clone()
    Xt2[3, 0] = -Xt2[3, 0]
    assert abo.update(m, Xt2, yt).update_path == "refit"


def test_gradient_gp_appends_and_falls_back():
    from oracle import grad_oracle as G
    d, N0, iters, ell, sf2, noise = 3, 30, 6, 0.8, 1.2, 1e-3
    p = d + 1
    N = N0 + iters
    X = synth.points(1, N, d)
    f = np.sin(2 * np.pi * X).sum(axis=1) / np.sqrt(d)
    gF = 2 * np.pi * np.cos(2 * np.pi * X) / np.sqrt(d)
    Ys = np.column_stack([f + 0.3, gF])
    mean_c = np.concatenate([[0.3], np.zeros(d)])
    Z = synth.points(2, 300, d)
    mk = lambda **kw: abo.GradientGP(sf2 * abo.with_lengthscale(FAMS[O.MATERN52](), ell), p, noise, mean=abo.gradConstMean(mean_c),
                                     n_max=64, **kw)
    m = abo.update(mk(incremental_update=True), X[:N0], Ys[:N0])
    for j in range(1, iters + 1):
        m = abo.update(m, X[:N0 + j], Ys[:N0 + j])
        assert m.update_path == "appended", j
    ref = abo.update(mk(), X, Ys)
    st = G.fit(O.MATERN52, ell, sf2, noise, mean_c, X, Ys)
    case = f"update/grad_fam{O.MATERN52}_d{d}_N{N0}+{iters}"
    mu_o, var_o = G.predict_grad(st, Z)
    check(case, "grad_mu", np.max(np.abs(abo.posterior_grad_mean(m, Z) - mu_o)), 1e-7)
    check(case, "grad_mu_vs_own_refit", np.max(np.abs(abo.posterior_grad_mean(m, Z) - abo.posterior_grad_mean(ref, Z))), 1e-7)
    check(case, "nlml_rel", abs(abo.nlml_fitted(m) - G.nlml(st)) / max(1.0, abs(G.nlml(st))), 1e-8)
    L, _, _ = abo.get_factor(m)
    Lr, _, _ = abo.get_factor(ref)
    check(case, "L_vs_own_refit", np.max(np.abs(L - Lr)), 1e-8)
    Yu = Ys.copy()
    Yu[4, 2] = np.nextafter(Yu[4, 2], -np.inf)                      # one gradient entry of the prefix
    out = abo.update(m, np.vstack([X, X[:1] + 0.01]), np.vstack([Yu, Ys[:1]]))
    assert out.update_path == "refit"


def test_sharded_update_matches_single_device_and_keeps_prev():
    d, N0, iters = 3, 150, 3
    X = synth.points(7, N0 + iters, d)
    y = synth.objective(X, 0.05)
    Z = synth.points(8, 2000, d)
    kern = 1.3 * abo.with_lengthscale(abo.Matern52Kernel(), 0.8)
    g = abo.update(abo.HipShardedGP(kern, 1e-3, devices=[0, 0], n_max=256, incremental_update=True), X[:N0], y[:N0])
    s = abo.update(abo.HipStandardGP(kern, 1e-3, n_max=256, incremental_update=True), X[:N0], y[:N0])
    prev = g
    mu_p, var_p = abo.mean_and_var(prev, Z)
    for j in range(1, iters + 1):
        g = abo.update(g, X[:N0 + j], y[:N0 + j])
        s = abo.update(s, X[:N0 + j], y[:N0 + j])
        assert g.update_path == s.update_path == "appended"
    mu_g, var_g = abo.mean_and_var(g, Z)
    mu_s, var_s = abo.mean_and_var(s, Z)
    np.testing.assert_array_equal(mu_g, mu_s)
    np.testing.assert_array_equal(var_g, var_s)
    acq = abo.ExpectedImprovement(0.01, float(np.min(y)))
    _, _, ti_g = abo.evaluate(acq, g, Z, k=10)
    _, _, ti_s = abo.evaluate(acq, s, Z, k=10)
    np.testing.assert_array_equal(ti_g, ti_s)
    mu_p2, var_p2 = abo.mean_and_var(prev, Z)
    np.testing.assert_array_equal(mu_p, mu_p2)
    np.testing.assert_array_equal(var_p, var_p2)
    assert abo.update(g, X[:N0 + iters], y[:N0 + iters]).update_path == "shared"


def test_plain_c_host_update_loop():
    """tests/c_update_harness.c: fit → 5 × abo_update → predict from a process without Python, checked against a refit"""
    src = os.path.join(ROOT, "tests", "c_update_harness.c")
    lib_dir = os.path.join(ROOT, "abstractbayesopt.jl_amd", "lib")
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "c_update_harness")
    # the HIP runtime the library names (NEEDED libamdhip64) lies beside the hipcc of the toolchain that built it
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", ""), "bin", "hipcc")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                           "-L", lib_dir, "-labo_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link," + rocm_lib, "-lm"])
    env = {k: v for k, v in os.environ.items() if k != "ABO_LIB_TEST_HOOKS"}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "c_update_harness ok" in r.stdout
