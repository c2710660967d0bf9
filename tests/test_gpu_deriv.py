"""abo_predict_deriv — the posterior of (f, ∇f) under a VALUE-ONLY model — through the C-ABI and the Python host (-m gpu), against
tests/deriv_oracle.py (tests/test_deriv_cpu.py checks that oracle against finite differences of independent ones).

Errors: mean max|Δμ_q|/max(1, |μ_q|); covariance max|ΔΣ_qq'|/sqrt(prior_q·prior_q'); score |Δs|/max(1, |s|) — all through
tests.parity_record.check: the project's hard bar 1e-6, and 100 × the error recorded on an MI355X in tests/golden/deriv_bounds.json
(floor 1e-13).  The record is a file of its own: tests/golden/parity_bounds.json is an existing yardstick and stays as it is."""
import ctypes as C
import json
import os
from functools import lru_cache

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import _lib, synth
from oracle import gp_oracle as O
from tests import deriv_oracle as D
from tests import parity_record
from tests.parity_record import check

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deriv_bounds.json")) as _f:
    parity_record.BOUNDS.update(json.load(_f))             # every case here is named deriv_*: nothing of parity_bounds.json is replaced

FAMS = {O.SE: abo.SqExponentialKernel, O.MATERN52: abo.Matern52Kernel, O.MATERN72: abo.ApproxMatern72Kernel}
SF2, MEAN_C, BETA = 1.7, 0.3, 2.0
M = 130
HARD = 1e-6
#         N,   d, noise, ell
CONFIGS = [(200, 3, 1e-2, 0.6), (128, 1, 1e-2, 0.6), (130, 32, 1e-2, 2.0)]
CASES = [(f, *c) for f in FAMS for c in CONFIGS]
NAN = float("nan")


def problem(N, d):
    X = synth.points(1, N, d)
    return X, synth.objective(X, 0.1) + 0.3


def queries(X, d):
    """130 points in [−0.1, 1.1]^d, the first three equal to training points"""
    z = np.random.default_rng(23).random((M, d)) * 1.2 - 0.1
    z[:3] = X[:3]
    return z


def model(family, ell, noise, **kw):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(FAMS[family](), ell), noise, mean=abo.ConstMean(MEAN_C), n_max=256, **kw)


def predict_deriv(h, z, beta=BETA, want=(True, True, True), d_arg=None, m_arg=None, null_z=False):
    """abo_predict_deriv on host arrays → (status, mu, cov, score), every output pre-filled with NaN (None where not asked for)"""
    z = np.ascontiguousarray(z, dtype=np.float64)
    m, d = z.shape
    p = d + 1
    mu = np.full((m, p), NAN) if want[0] else None
    cov = np.full((m, p, p), NAN) if want[1] else None
    sc = np.full(m, NAN) if want[2] else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    st = _lib.lib().abo_predict_deriv(h, None if null_z else z.ctypes.data, m if m_arg is None else m_arg, d if d_arg is None else d_arg,
                                      _lib.HOST, float(beta), ptr(mu), ptr(cov), ptr(sc), _lib.HOST)
    return st, mu, cov, sc


def ok(r):
    _lib.check(r[0])
    return r[1:]


def bits(*xs):
    return b"".join(np.ascontiguousarray(x, dtype=np.float64).tobytes() for x in xs)


def errors(got, ref):
    """(mean, covariance, score) errors of (mu, cov, score) against the oracle's (mu, cov, score, prior)"""
    mu, cov, sc = got
    rmu, rcov, rsc, prior = ref
    scale = np.sqrt(np.outer(prior, prior))
    return (float(np.max(np.abs(mu - rmu) / np.maximum(1.0, np.abs(rmu)))), float(np.max(np.abs(cov - rcov) / scale[None])),
            float(np.max(np.abs(sc - rsc) / np.maximum(1.0, np.abs(rsc)))))


@lru_cache(maxsize=None)
def case(family, N, d, noise, ell):
    """everything the tests of one case compare, computed once and left unchanged"""
    X, y = problem(N, d)
    z = queries(X, d)
    m = abo.update(model(family, ell, noise, contraction="fp64"), X, y)
    out = {"X": X, "y": y, "z": z, "m": m}
    out["got"] = ok(predict_deriv(m._require(), z))
    out["again"] = ok(predict_deriv(m._require(), z))
    out["one"] = ok(predict_deriv(m._require(), z[:1]))
    out["ref"] = D.posterior(family, ell, SF2, noise, MEAN_C, X, y, z, BETA)
    return out


def name_of(family, N, d, noise, ell):
    return f"deriv_fam{family}_N{N}_d{d}"


def held(nm, got, ref, suffix=""):
    e = errors(got, ref)
    print(f"{nm}{suffix}: mean {e[0]:.3e}, cov {e[1]:.3e}, score {e[2]:.3e}")
    for metric, v in zip(("mean", "cov", "score"), e):
        check(nm, metric + suffix, v, HARD)


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_parity_with_the_oracle(family, N, d, noise, ell):
    c = case(family, N, d, noise, ell)
    nm = name_of(family, N, d, noise, ell)
    held(nm, c["got"], c["ref"])
    # M = 1: the first point alone — the same bits as in the batch, and the oracle's
    assert bits(*c["one"]) == bits(c["got"][0][:1], c["got"][1][:1], c["got"][2][:1])
    held(nm, c["one"], tuple(a[:1] for a in c["ref"][:3]) + (c["ref"][3],), "_m1")
    # symmetric blocks
    assert np.array_equal(c["got"][1], np.swapaxes(c["got"][1], 1, 2))


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_function_output_agrees_with_abo_predict(family, N, d, noise, ell):
    c = case(family, N, d, noise, ell)
    nm = name_of(family, N, d, noise, ell)
    mu, var = abo.mean_and_var(c["m"], c["z"])
    e_mu = float(np.max(np.abs(c["got"][0][:, 0] - mu) / np.maximum(1.0, np.abs(mu))))
    e_var = float(np.max(np.abs(c["got"][1][:, 0, 0] - var))) / SF2
    print(f"{nm}: mu0 vs abo_predict {e_mu:.3e}, var0 vs abo_predict {e_var:.3e}")
    check(nm, "mu0_vs_predict", e_mu, HARD)
    check(nm, "var0_vs_predict", e_var, HARD)
    assert c["m"].timings()["contraction_engine"] == _lib.CONTRACT_FP64


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_determinism_chunking_null_outputs_and_memory_space(family, N, d, noise, ell):
    import torch
    c = case(family, N, d, noise, ell)
    h, z = c["m"]._require(), c["z"]
    ref = bits(*c["got"])
    assert bits(*c["again"]) == ref
    # 64 points per chunk: three chunks, the last one of two points
    mc = abo.update(model(family, ell, noise, contraction="fp64", chunk=64), c["X"], c["y"])
    assert bits(*ok(predict_deriv(mc._require(), z))) == ref
    # the int8 engine asked for: the call still runs on the fp64 GEMM and says so
    mi = abo.update(model(family, ell, noise, contraction="int8"), c["X"], c["y"])
    assert bits(*ok(predict_deriv(mi._require(), z))) == ref
    assert mi.timings()["contraction_engine"] == _lib.CONTRACT_FP64
    for drop in range(3):
        want = tuple(i != drop for i in range(3))
        r = ok(predict_deriv(h, z, want=want))
        assert r[drop] is None
        assert bits(*[a for a in r if a is not None]) == bits(*[a for i, a in enumerate(c["got"]) if i != drop])
    zd = torch.from_numpy(z).cuda()
    p = d + 1
    mu_d = torch.full((M, p), NAN, dtype=torch.float64, device="cuda")
    cov_d = torch.full((M, p, p), NAN, dtype=torch.float64, device="cuda")
    sc_d = torch.full((M,), NAN, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().abo_predict_deriv(h, zd.data_ptr(), M, d, _lib.DEVICE, BETA, mu_d.data_ptr(), cov_d.data_ptr(), sc_d.data_ptr(),
                                            _lib.DEVICE))
    assert bits(mu_d.cpu().numpy(), cov_d.cpu().numpy(), sc_d.cpu().numpy()) == ref
    # M = 0: ABO_OK, nothing written
    st, mu0, cov0, sc0 = predict_deriv(h, z[:2], m_arg=0)
    assert st == _lib.ABO_OK and np.all(np.isnan(mu0)) and np.all(np.isnan(cov0)) and np.all(np.isnan(sc0))


@pytest.mark.parametrize("family", list(FAMS))
def test_views_after_append_and_remove(family):
    N, d, noise, ell = 200, 3, 1e-2, 0.6
    c = case(family, N, d, noise, ell)
    X, y, z = c["X"], c["y"], c["z"][:40]
    xn = np.array([0.31, 0.62, 0.47])
    yn = 0.45
    ma = abo.append(c["m"], xn, yn)
    ref = D.posterior(family, ell, SF2, noise, MEAN_C, np.vstack([X, xn]), np.append(y, yn), z, BETA)
    held(f"deriv_fam{family}_views", ok(predict_deriv(ma._require(), z)), ref, "_append")
    # the parent still answers for its own N points
    assert bits(*ok(predict_deriv(c["m"]._require(), c["z"]))) == bits(*c["got"])
    idx = [5, 77, 150]
    mr = abo.remove_points(c["m"], idx)
    keep = np.setdiff1d(np.arange(N), idx)
    ref = D.posterior(family, ell, SF2, noise, MEAN_C, X[keep], y[keep], z, BETA)
    held(f"deriv_fam{family}_views", ok(predict_deriv(mr._require(), z)), ref, "_remove")


@pytest.mark.parametrize("family", list(FAMS))
def test_python_host(family):
    N, d, noise, ell = 200, 3, 1e-2, 0.6
    c = case(family, N, d, noise, ell)
    m, z = c["m"], c["z"]
    rmu, rcov, rsc, prior = c["ref"]
    nm = f"deriv_fam{family}_host"
    # by outputs: entry q·M + j
    gm, gv = abo.posterior_grad_mean(m, z), abo.posterior_grad_var(m, z)
    assert gm.shape == gv.shape == (M * (d + 1),)
    check(nm, "grad_mean", float(np.max(np.abs(gm - rmu.T.reshape(-1)) / np.maximum(1.0, np.abs(rmu.T.reshape(-1))))), HARD)
    rvar = np.einsum("jqq->qj", rcov).reshape(-1)
    check(nm, "grad_var", float(np.max(np.abs(gv - rvar) / np.repeat(prior, M))), HARD)
    gc = abo.posterior_grad_cov(m, z)
    assert gc.shape == (M, d + 1, d + 1) and abo.posterior_grad_cov(m, z[:1]).shape == (d + 1, d + 1)
    check(nm, "grad_cov", float(np.max(np.abs(gc - rcov) / np.sqrt(np.outer(prior, prior))[None])), HARD)
    acq = abo.GradientNormUCB(BETA)
    s = acq(m, z)
    check(nm, "score", float(np.max(np.abs(s - rsc) / np.maximum(1.0, np.abs(rsc)))), HARD)
    scores, tv, ti = abo.evaluate(acq, m, z, k=10)
    assert np.array_equal(scores, s)
    ov, oi = O.top_k(rsc, 10)
    assert np.array_equal(ti, oi)
    check(nm, "top_k_values", float(np.max(np.abs(tv - ov) / np.maximum(1.0, np.abs(ov)))), HARD)
    assert abo.evaluate(acq, m, z, k=0, return_scores=False) == (None, None, None)


def test_python_host_ard():
    family, N, d, noise = O.MATERN52, 200, 3, 1e-2
    ells = (0.3, 0.6, 1.2)
    X, y = problem(N, d)
    z = queries(X, d)
    m = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(FAMS[family](), ells), noise, mean=abo.ConstMean(MEAN_C)), X, y)
    rmu, rcov, rsc, prior = D.posterior_ard(family, ells, SF2, noise, MEAN_C, X, y, z, BETA)
    mu, cov, sc = abo.posterior_grad_cov(m, z, beta=BETA, return_all=True)
    held("deriv_ard_host", (mu, cov, sc), (rmu, rcov, rsc, prior))
    gm = abo.posterior_grad_mean(m, z)
    assert np.array_equal(gm, mu.T.reshape(-1))
    assert np.array_equal(abo.GradientNormUCB(BETA)(m, z), sc)


def test_refusals():
    """each returns ABO_EINVAL, names the call in abo_last_error and leaves the outputs alone"""
    L = _lib.lib()
    c = case(O.SE, 200, 3, 1e-2, 0.6)
    z = c["z"][:4]

    def refused(what, h, zz, **kw):
        st, mu, cov, sc = predict_deriv(h, zz, **kw)
        assert st == _lib.ABO_EINVAL, what
        assert "abo_predict_deriv" in _lib.last_error(), (what, _lib.last_error())
        assert np.all(np.isnan(mu)) and np.all(np.isnan(cov)) and np.all(np.isnan(sc)), what

    Xg = synth.points(2, 12, 2)
    yg = np.column_stack([np.sin(Xg.sum(1)), np.cos(Xg.sum(1)), np.cos(Xg.sum(1))])
    mg = abo.update(abo.HipGradientGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), 0.6), 3, 1e-2), Xg, yg)
    refused("a gradient-enhanced handle", mg._require(), np.zeros((4, 2)))
    hp = C.c_void_p()
    prm = model(O.SE, 0.6, 1e-2)._params()
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    try:
        refused("an unfitted handle", hp.value, z)
    finally:
        L.abo_destroy(hp.value)
    refused("a dimension mismatch", c["m"]._require(), np.zeros((4, 2)))
    X1, y1 = problem(40, 3)
    m32 = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern32Kernel(), 0.6), 1e-2), X1, y1)
    refused("Matérn-3/2", m32._require(), z)
    X33, y33 = problem(40, 33)
    m33 = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.SqExponentialKernel(), 2.0), 1e-2), X33, y33)
    refused("a d = 33 model", m33._require(), np.zeros((4, 33)))
    refused("M < 0", c["m"]._require(), z, m_arg=-1)
    refused("a null Z", c["m"]._require(), z, null_z=True)
    # the Python host turns the status into ValueError
    with pytest.raises(ValueError, match="abo_predict_deriv"):
        abo.posterior_grad_mean(m32, z)
