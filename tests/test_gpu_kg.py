"""Knowledge gradient over a discrete decision set on the device: the row kernel through abo_test_kg_lines (lines handed in, no model),
abo_acq_kg, and the Python host on top of it.

The checker is tests/kg_oracle.py.  Hook cases: Mb = 1, 2, 63, 64, 65, 257 (five rows each, duplicate slopes and intercepts planted, a
leading dimension beyond Mb) and 8192 (two rows: the full-size sort, 128 KiB of LDS); the tangents of a parabola (every line on the
envelope) and one dominating line (the scan pops the whole stack) at 257 and 8192; a row with a NaN; the own line given and not.
Model cases: kg_oracle.GP_CASES, Za (130) against Zb (257).

Errors are |KG_gpu − KG_oracle|/√σ_f² (the hook's lines are O(1): the scale is 1), held under the project's 1e-6 bar and under 100 × the
error recorded on an MI355X in tests/golden/kg_bounds.json (floor 1e-13): tests.parity_record.check.  Envelope counts must match
exactly, except on rows where the checker itself compared two breakpoints within 4 ulp; such rows stay below 1 % of a case."""
import ctypes as C
import json
import math
import os
from functools import lru_cache

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import _lib, synth
from abstractbayesopt.jl_amd import surrogate as S
from oracle import gp_oracle as O
from tests import kg_oracle as K
from tests import parity_record
from tests.parity_record import check

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kg_bounds.json")) as _f:
    parity_record.BOUNDS.update(json.load(_f))             # every case here is named kg_*: nothing of parity_bounds.json is replaced

FAMS = {O.SE: abo.SqExponentialKernel, O.MATERN52: abo.Matern52Kernel, O.MATERN72: abo.ApproxMatern72Kernel, O.MATERN32: abo.Matern32Kernel}
SF2, MEAN_C, MA, MB = K.SF2, K.MEAN_C, K.MA, K.MB
HARD = 1e-6
SCALE = math.sqrt(SF2)
CASES = [(f, *K.GP_CASES[0]) for f in FAMS] + [(O.MATERN52, *c) for c in K.GP_CASES[1:]]
FORMS = ("rect", "self", "sym")
NOISES = (-1.0, 0.0, 0.05)


def bits(*xs):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in xs)


# ---- the row kernel on given lines -------------------------------------------------------------------------
def run_lines(a, B, self_a=None, self_b=None, pad=3):
    """abo_test_kg_lines on device copies of the lines (rows of B in a buffer of leading dimension Mb + pad) → (val, nenv)"""
    import torch
    a, B = np.ascontiguousarray(a, dtype=np.float64), np.asarray(B, dtype=np.float64)
    ma, mb = B.shape
    Bp = np.full((ma, mb + pad), 7.5)
    Bp[:, :mb] = B
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    at, Bt, sat, sbt = dev(a), dev(Bp), dev(self_a), dev(self_b)
    val = torch.full((ma,), -3.0, dtype=torch.float64, device="cuda")
    nenv = torch.full((ma,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().abo_test_kg_lines(0, ptr(at), ptr(Bt), mb + pad, ma, mb, ptr(sat), ptr(sbt), ptr(val), ptr(nenv)))
    return val.cpu().numpy(), nenv.cpu().numpy().astype(np.int64)


def hold(name, got, want):
    """values under the bar through the record; counts exact but on the checker's tie rows (< 1 % of the case)"""
    (val, nenv), (rv, rn, tie) = got, want
    fin = np.isfinite(rv)
    assert np.array_equal(np.isnan(val), np.isnan(rv))
    e = float(np.max(np.abs(val[fin] - rv[fin]))) if fin.any() else 0.0
    print(name, {"val": e, "ties": int(tie.sum()), "median_env": float(np.median(rn))})
    assert np.all(val[fin] >= 0.0)
    check(name, "val", e, HARD)
    assert tie.sum() <= 0.01 * len(tie)
    assert np.array_equal(nenv[~tie], rn[~tie])


def random_lines(mb, ma, seed):
    rng = np.random.default_rng(seed)
    a, B = rng.standard_normal(mb), rng.standard_normal((ma, mb))
    if mb >= 5:
        B[:, 1] = B[:, 3]                       # duplicate slopes in every row …
        B[:, mb - 1] = B[:, 0]
        a[2] = a[4]                             # … and a duplicate intercept
        B[0, : mb // 2] = B[0, 0]               # one row with half of its slopes equal
    return a, B


@pytest.mark.parametrize("mb", [1, 2, 63, 64, 65, 257])
def test_lines_against_the_oracle(mb):
    a, B = random_lines(mb, 5, 100 + mb)
    hold(f"kg_lines_Mb{mb}", run_lines(a, B), K.kg_rows(a, B))
    rng = np.random.default_rng(mb)
    sa, sb = rng.standard_normal(5), rng.standard_normal(5)
    sb[1] = B[1, 0]                             # an own line with the slope of another line of its row
    hold(f"kg_lines_Mb{mb}_self", run_lines(a, B, sa, sb), K.kg_rows(a, B, sa, sb))
    if mb == 1:
        v, n = run_lines(a, B)
        assert np.all(v == 0.0) and np.all(n == 1)


def test_lines_full_size():
    """Mb = 8192: two rows through the 8192-wide sort"""
    a, B = random_lines(8192, 2, 8192)
    hold("kg_lines_Mb8192", run_lines(a, B), K.kg_rows(a, B))


@pytest.mark.parametrize("mb", [257, 8192])
def test_parabola_tangents_and_a_dominating_line(mb):
    rng = np.random.default_rng(mb + 1)
    b = np.linspace(-3.0, 3.0, mb)
    a = -0.5 * b * b
    perm = rng.permutation(mb)
    B = np.stack([b[perm], b[perm][::-1] * 0.5])          # the tangents, shuffled in memory, and a second row beside them
    got, want = run_lines(a[perm], B, pad=1), K.kg_rows(a[perm], B)
    assert want[1][0] == mb                              # every tangent is on the envelope
    hold(f"kg_parabola_Mb{mb}", got, want)
    assert got[1][0] == mb
    # one steep line far above the rest (its breakpoints lie below −3e8), first in memory and last in the order: it pops all but the
    # line of the lowest slope
    a2, b2 = rng.standard_normal(mb), rng.uniform(-1.0, 1.0, mb)
    a2[0], b2[0] = 1e9, 2.0
    want2 = K.kg_rows(a2, b2[None, :])
    assert want2[1][0] == 2
    hold(f"kg_dominating_Mb{mb}", run_lines(a2, b2[None, :]), want2)


def test_equal_slopes_and_a_row_with_a_nan():
    a, B = random_lines(65, 4, 9)
    B[1, :] = 0.25                               # all slopes equal: exactly 0.0, one line
    B[2, 17] = np.nan
    val, nenv = run_lines(a, B)
    rv, rn, tie = K.kg_rows(a, B)
    assert val[1] == 0.0 and nenv[1] == 1
    assert np.isnan(val[2]) and nenv[2] == 0 and np.isnan(rv[2])
    hold("kg_lines_nan_row", (val, nenv), (rv, rn, tie))
    a[5] = np.inf                                # a non-finite intercept spoils every row
    val, nenv = run_lines(a, B)
    assert np.all(np.isnan(val)) and np.all(nenv == 0)


# ---- abo_acq_kg ------------------------------------------------------------------------------------------------
def model(family, ell, noise, **kw):
    return abo.HipStandardGP(SF2 * abo.with_lengthscale(FAMS[family](), ell), noise, mean=abo.ConstMean(MEAN_C), n_max=256, **kw)


def acq_kg(m, za, zb=None, noise=-1.0, flags=0, k=0, idx_base=0, mb_arg=None, d_arg=None, want_scores=True):
    """abo_acq_kg on host arrays → (status, scores, top_val, top_idx), every output pre-filled"""
    za = np.ascontiguousarray(za, dtype=np.float64)
    ma, d = za.shape
    zb = None if zb is None else np.ascontiguousarray(zb, dtype=np.float64)
    mb = 0 if zb is None else zb.shape[0]
    sc = np.full(ma, np.nan)
    tv, ti = np.full(max(k, 1), np.nan), np.full(max(k, 1), -5, dtype=np.int64)
    st = _lib.lib().abo_acq_kg(m._require(), za.ctypes.data, ma, None if zb is None else zb.ctypes.data, mb if mb_arg is None else mb_arg,
                               d if d_arg is None else d_arg, _lib.HOST, noise, flags, idx_base, sc.ctypes.data if want_scores else None, k,
                               tv.ctypes.data if k > 0 else None, ti.ctypes.data if k > 0 else None, _lib.HOST)
    return st, sc, tv[:k], ti[:k]


def ok(r):
    _lib.check(r[0])
    return r[1:]


def by_form(m, za, zb, form, noise=-1.0, **kw):
    return acq_kg(m, za, None if form == "sym" else zb, noise=noise, flags=_lib.KG_SELF if form == "self" else 0, **kw)


@lru_cache(maxsize=None)
def case(family, N, d, noise, ell):
    """the model of a case and the checker's posterior quantities, computed once and left unchanged"""
    from tests import cov_oracle as CO
    X, y = K.gp_problem(N, d)
    za, zb = K.gp_queries(d)
    m = abo.update(model(family, ell, noise), X, y)
    mu_a, cov_aa = CO.mean_and_cov(family, ell, SF2, noise, MEAN_C, X, y, za)
    mu_b, _ = CO.mean_and_cov(family, ell, SF2, noise, MEAN_C, X, y, zb)
    cov_ab = CO.posterior_cov(family, ell, SF2, noise, X, za, zb)
    return {"X": X, "y": y, "za": za, "zb": zb, "m": m, "mu_a": mu_a, "mu_b": mu_b, "cov_aa": cov_aa, "cov_ab": cov_ab, "noise": noise}


@lru_cache(maxsize=None)
def reference(family, N, d, noise, ell, form, nz):
    c = case(family, N, d, noise, ell)
    nz = c["noise"] if nz < 0 else nz
    v = np.diag(c["cov_aa"])
    if form == "sym":
        return K.kg_from_posterior(c["mu_a"], c["cov_aa"], v, nz)
    return K.kg_from_posterior(c["mu_b"], c["cov_ab"], v, nz, mu_a=c["mu_a"] if form == "self" else None)


def name_of(family, N, d):
    return f"kg_fam{family}_N{N}_d{d}"


@pytest.mark.parametrize("family,N,d,noise,ell", CASES)
def test_parity_with_the_oracle(family, N, d, noise, ell):
    c = case(family, N, d, noise, ell)
    errs = {}
    for form in FORMS:
        for nz in NOISES:
            sc = ok(by_form(c["m"], c["za"], c["zb"], form, noise=nz))[0]
            rv = reference(family, N, d, noise, ell, form, nz)[0]
            assert np.all(np.isfinite(sc)) and np.all(sc >= 0.0)
            errs[f"{form}_noise{nz:g}"] = float(np.max(np.abs(sc - rv))) / SCALE
    print(name_of(family, N, d), errs)
    for k, e in errs.items():
        check(name_of(family, N, d), k, e, HARD)


@pytest.mark.parametrize("form", FORMS)
def test_top_k_idx_base_and_determinism(form):
    c = case(O.MATERN52, *K.GP_CASES[0])
    m, za, zb = c["m"], c["za"], c["zb"]
    sc, _, _ = ok(by_form(m, za, zb, form))
    for k in (10, MA):
        sc2, tv, ti = ok(by_form(m, za, zb, form, k=k, idx_base=1000))
        assert bits(sc2) == bits(sc)                                    # two calls: the same bits
        rv, ri = K.top_k(sc, k)
        assert np.array_equal(ti, ri + 1000) and bits(tv) == bits(rv)
    # the selection alone, and more pairs than candidates
    _, tv, ti = ok(by_form(m, za, zb, form, k=MA + 2, want_scores=False))
    assert np.array_equal(ti[:MA], K.top_k(sc, MA)[1]) and np.all(ti[MA:] == -1) and np.all(np.isnan(tv[MA:]))


def test_device_space_equals_host_space():
    import torch
    c = case(O.MATERN52, *K.GP_CASES[0])
    m, d = c["m"], c["za"].shape[1]
    za, zb = torch.from_numpy(c["za"]).cuda(), torch.from_numpy(c["zb"]).cuda()
    sc = torch.full((MA,), float("nan"), dtype=torch.float64, device="cuda")
    tv = torch.full((10,), float("nan"), dtype=torch.float64, device="cuda")
    ti = torch.full((10,), -5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().abo_acq_kg(m._require(), za.data_ptr(), MA, zb.data_ptr(), MB, d, _lib.DEVICE, -1.0, _lib.KG_SELF, 0, sc.data_ptr(), 10,
                                     tv.data_ptr(), ti.data_ptr(), _lib.DEVICE))
    h = ok(by_form(m, c["za"], c["zb"], "self", k=10))
    assert bits(sc.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()) == bits(*h)


@pytest.mark.parametrize("family", [O.SE, O.MATERN52])
def test_engine_setting_changes_nothing(family):
    cfg = K.GP_CASES[0]
    c = case(family, *cfg)
    want = {form: ok(by_form(c["m"], c["za"], c["zb"], form))[0] for form in FORMS}
    for eng in ("fp64", "int8"):
        m = abo.update(model(family, cfg[3], cfg[2], contraction=eng), c["X"], c["y"])
        abo.posterior_var(m, c["za"])                           # the handle's own engine has run first
        for form in FORMS:
            assert bits(ok(by_form(m, c["za"], c["zb"], form))[0]) == bits(want[form]), (eng, form)


def test_views():
    """a parent returns the same bits before and after a child was appended in place; the child agrees with the checker on 131 points"""
    family, (N, d, noise, ell) = O.MATERN52, K.GP_CASES[0]
    c = case(family, N, d, noise, ell)
    X, y, za, zb = c["X"], c["y"], c["za"], c["zb"]
    m = abo.update(model(family, ell, noise), X, y)
    before = {f: ok(by_form(m, za, zb, f))[0] for f in FORMS}
    xs, ys = np.array([0.37, 0.52, 0.81]), 0.9
    m2 = abo.append(m, xs, ys)
    for f in FORMS:
        assert bits(ok(by_form(m, za, zb, f))[0]) == bits(before[f])
    X2, y2 = np.vstack([X, xs[None, :]]), np.append(y, ys)
    e = {}
    for f in FORMS:
        rv = K.kg_model(family, ell, SF2, noise, MEAN_C, X2, y2, za, None if f == "sym" else zb, include_self=f == "self")[0]
        e[f] = float(np.max(np.abs(ok(by_form(m2, za, zb, f))[0] - rv))) / SCALE
    print("kg_view131", e)
    for f, v in e.items():
        check("kg_view131", f, v, HARD)
    for f in FORMS:
        assert bits(ok(by_form(m, za, zb, f))[0]) == bits(before[f])      # the parent once more, behind the child's own calls


def test_a_candidate_on_a_training_point_of_a_noise_free_model_is_exactly_zero():
    """N = 40 at d = 2 with ℓ = 0.05: K is close to σ_f²·I, the factorisation needs no jitter (L₀₀² = σ_f² to rounding says so) and the
    latent variance at a training point is a rounding error, far below the 1e-12 floor: with the factor's own noise (0) the row is 0.0"""
    X, y = K.gp_problem(40, 2)
    m = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), 0.05), 0.0, mean=abo.ConstMean(MEAN_C), jitter=1e-8), X, y)
    L00 = abo.get_factor(m)[0][0, 0]
    assert abs(L00 * L00 - SF2) < 1e-12, "the factor was built with jitter: the case needs another length scale"
    za, zb = K.gp_queries(2)
    za = za.copy()
    za[7], za[50] = X[3], X[39]
    for form in FORMS:
        sc = ok(by_form(m, za, zb, form))[0]
        assert sc[7] == 0.0 and sc[50] == 0.0 and not np.signbit(sc[7]), form
        assert np.all(np.isfinite(sc)) and np.all(sc >= 0.0) and np.any(sc > 0.0), form


def last_error_after(st, want=_lib.ABO_EINVAL):
    assert st == want
    text = _lib.last_error()
    assert text.strip()
    return text


def test_refusals():
    """every refusal returns its status with a text in abo_last_error and leaves the outputs untouched"""
    c = case(O.MATERN52, *K.GP_CASES[0])
    m, za, zb = c["m"], c["za"], c["zb"]
    d = za.shape[1]
    seen = []

    def refused(r, word, want=_lib.ABO_EINVAL):
        assert word in last_error_after(r[0], want), word
        seen.append(r)

    refused(acq_kg(m, np.zeros((8193, d)), None), "Ma")
    refused(acq_kg(m, za, np.zeros((8193, d))), "Mb")
    refused(acq_kg(m, za, None, mb_arg=MA - 1), "Mb")
    refused(acq_kg(m, za, None, flags=_lib.KG_SELF), "ABO_KG_SELF")
    refused(acq_kg(m, za, zb, flags=2), "flags")
    refused(acq_kg(m, za, zb, noise=float("nan")), "noise")
    refused(acq_kg(m, za, zb, noise=float("inf")), "noise")
    refused(acq_kg(m, za, zb, k=-1), "k")
    refused(acq_kg(m, za, zb, d_arg=d - 1), "DimensionMismatch", _lib.ABO_EDIM)
    L = _lib.lib()
    sc = np.full(MA, np.nan)
    assert "Ma" in last_error_after(L.abo_acq_kg(m._require(), za.ctypes.data, 0, None, 0, d, _lib.HOST, -1.0, 0, 0, sc.ctypes.data, 0, None, None, _lib.HOST))
    assert "top_val" in last_error_after(L.abo_acq_kg(m._require(), za.ctypes.data, MA, None, 0, d, _lib.HOST, -1.0, 0, 0, sc.ctypes.data, 3, None, None, _lib.HOST))
    assert "null" in last_error_after(L.abo_acq_kg(None, za.ctypes.data, MA, None, 0, d, _lib.HOST, -1.0, 0, 0, sc.ctypes.data, 0, None, None, _lib.HOST))
    hp = C.c_void_p()
    prm = model(O.MATERN52, 0.3, 1e-2)._params()
    _lib.check(L.abo_create(C.byref(prm), C.byref(hp)))
    try:
        assert "not conditioned" in last_error_after(L.abo_acq_kg(hp.value, za.ctypes.data, MA, None, 0, d, _lib.HOST, -1.0, 0, 0, sc.ctypes.data, 0, None, None, _lib.HOST))
    finally:
        L.abo_destroy(hp.value)
    Xg = synth.points(2, 20, d)
    g = abo.update(abo.HipGradientGP(abo.with_lengthscale(abo.Matern52Kernel(), 0.6), d + 1, 1e-2), Xg, np.zeros((20, d + 1)))
    assert "gradient" in last_error_after(L.abo_acq_kg(g._require(), za.ctypes.data, MA, None, 0, d, _lib.HOST, -1.0, 0, 0, sc.ctypes.data, 0, None, None, _lib.HOST))
    with pytest.raises(TypeError, match="gradient"):
        abo.knowledge_gradient(g, za)
    assert np.all(np.isnan(sc))
    for _, s, tv, ti in seen:
        assert np.all(np.isnan(s)) and np.all(np.isnan(tv)) and np.all(ti == -5)
    assert bits(ok(by_form(m, za, zb, "self"))[0]) == bits(ok(by_form(m, za, zb, "self"))[0])     # the handle still serves


# ---- the Python host -------------------------------------------------------------------------------------------
def test_python_host_isotropic():
    family, (N, d, noise, ell) = O.MATERN52, K.GP_CASES[0]
    c = case(family, N, d, noise, ell)
    m, za, zb = c["m"], c["za"], c["zb"]
    assert bits(abo.knowledge_gradient(m, za, zb)) == bits(ok(by_form(m, za, zb, "self"))[0])
    assert bits(abo.knowledge_gradient(m, za, zb, include_self=False, noise=0.05)) == bits(ok(by_form(m, za, zb, "rect", noise=0.05))[0])
    sc, tv, ti = abo.knowledge_gradient(m, za, k=10)
    assert bits(sc, tv, ti) == bits(*ok(by_form(m, za, zb, "sym", k=10)))
    e = float(np.max(np.abs(sc - reference(family, N, d, noise, ell, "sym", -1.0)[0]))) / SCALE
    check("kg_python_iso", "sym", e, HARD)
    kg = abo.KnowledgeGradient(decision=zb)
    assert bits(kg(m, za)) == bits(abo.knowledge_gradient(m, za, zb))
    assert abo.update(kg, c["y"], m) is kg
    s2, tv2, ti2 = abo.evaluate(kg, m, za, k=10)
    assert bits(s2) == bits(kg(m, za)) and np.array_equal(ti2, K.top_k(s2, 10)[1])
    # decision="train": the model's own points, refreshed by update
    kt = abo.update(abo.KnowledgeGradient(decision="train"), c["y"], m)
    assert np.array_equal(kt.points, c["X"]) and bits(kt(m, za)) == bits(abo.knowledge_gradient(m, za, c["X"]))
    # tensors in, tensors out
    import torch
    zt = torch.from_numpy(za).cuda()
    st, tvt, tit = abo.knowledge_gradient(m, zt, torch.from_numpy(zb).cuda(), k=10)
    assert st.is_cuda and bits(st.cpu().numpy(), tvt.cpu().numpy(), tit.cpu().numpy()) == bits(*ok(by_form(m, za, zb, "self", k=10)))


def test_python_host_chunked(monkeypatch):
    """the chunked route with the chunk size brought down to 64: 130 candidates in three calls, the selections merged on the host"""
    c = case(O.MATERN52, *K.GP_CASES[0])
    m, za, zb = c["m"], c["za"], c["zb"]
    whole = abo.knowledge_gradient(m, za, zb, k=MA)
    monkeypatch.setattr(S, "KG_CHUNK", 64)
    for k in (10, 70, MA):
        sc, tv, ti = abo.knowledge_gradient(m, za, zb, k=k)
        assert bits(sc) == bits(whole[0])                       # a row's value does not depend on the rows beside it
        assert np.array_equal(ti, whole[2][:k]) and bits(tv) == bits(whole[1][:k])
    assert bits(abo.knowledge_gradient(m, za, zb)) == bits(whole[0])


def test_python_host_ard():
    X, y = K.gp_problem(130, 3)
    za, zb = K.gp_queries(3)
    ell = np.array([0.2, 0.26, 0.33])
    ard = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), list(ell)), 1e-2, mean=abo.ConstMean(MEAN_C)), X, y)
    iso = abo.update(abo.HipStandardGP(SF2 * abo.with_lengthscale(abo.Matern52Kernel(), 1.0), 1e-2, mean=abo.ConstMean(MEAN_C)), X / ell, y)
    got = abo.knowledge_gradient(ard, za, zb)
    assert bits(got) == bits(abo.knowledge_gradient(iso, za / ell, zb / ell))
    rv = K.kg_model(O.MATERN52, 1.0, SF2, 1e-2, MEAN_C, X / ell, y, za / ell, zb / ell, include_self=True)[0]
    check("kg_python_ard", "self", float(np.max(np.abs(got - rv))) / SCALE, HARD)
    assert bits(abo.KnowledgeGradient()(ard, za)) == bits(abo.knowledge_gradient(iso, za / ell))
    with pytest.raises(abo.DimensionMismatch):
        abo.knowledge_gradient(ard, za[:, :2])
