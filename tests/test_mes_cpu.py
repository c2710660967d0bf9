"""Max-value entropy search (ABO_ACQ_MES = 6) without a GPU: the CPU restatement of MES that the GPU tests compare against
(tests/test_gpu_mes.py imports it from here) against the mpmath table tests/golden/mes_kat.npz, its sign and monotonicity, the constants
of the boundary, and the Python and Julia hosts' plumbing on a stubbed library.

The restatement (NumPy + scipy.special.erfcx) is  MES = (1/S)·Σ_s a(γ_s),  γ_s = (μ − y*_s)/σ,  a(γ) = γ·φ/(2Φ) − log Φ, 0 for
σ² ≤ 1e-12, with a in three ranges of γ (directly for γ > −1, through erfcx down to −32, the asymptotic series of the Mills ratio
below): the arithmetic of csrc/abo_acq_dev.h: mes_a."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.special import erfc, erfcx

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import acquisition as A
from abstractbayesopt.jl_amd import thompson as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "abo_hip.h")
JULIA = os.path.join(ROOT, "integration", "julia", "MaxValueEntropySearch.jl")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mes_kat.npz")
MES = 6
SEAMS = (-32.0, -1.0, 0.0)             # the cut points of mes_a

# Bars of the restatement against the table (fp64, libm good to a few ulp, u = 2⁻⁵³ = 1.1e-16):
#   value    a' is bounded by 1 and γ carries 3 roundings: 3u·|γ|·|a'| ≤ 3u·max(1, …) — nothing; the erfcx range forms (γ/2q)·w with
#            w = 1 + γq ≈ 1/γ² from a sum near −1 + 1: at the −32 seam |γ/2q| ≈ 512 times (erfcx, a product, the sum: ≤ 6u) = 3.4e-13
#            absolute under |ref| ≈ 4.4: 8e-14 relative to max(1, |ref|).  The bar is the ceiling of the device test, 1e-12.
#   partials the bracket 1 + (γ/q)·w ≈ 2/γ² loses the same 10 bits once more: 2¹⁰·512·6u ≈ 3.5e-10 relative at the −32 seam; the bar
#            is 1e-8, asserted for γ ≥ −64 as in the device test; below, finiteness and sign.
VALUE_BAR, PARTIAL_BAR = 1e-12, 1e-8


def mes_a(g):
    """(a(γ), a'(γ)) in NumPy, the three ranges of csrc/abo_acq_dev.h: mes_a"""
    g = np.asarray(g, dtype=np.float64)
    a, da = np.full_like(g, np.nan), np.full_like(g, np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        s = g > -1.0
        x = g[s]
        cdf = 0.5 * erfc(-x * 0.7071067811865476)
        r = np.exp(-0.5 * x * x) * 0.3989422804014327 / cdf
        t = x * r
        da[s] = -0.5 * (r + t * (x + r))
        a[s] = 0.5 * t - np.where(x > 0.0, np.log1p(-0.5 * erfc(x * 0.7071067811865476)), np.log(cdf))
        s = (g <= -1.0) & (g > -32.0)
        x = g[s]
        q = 1.2533141373155003 * erfcx(-x * 0.7071067811865476)              # Φ/φ
        w, gr = 1.0 + x * q, x / q
        da[s] = -0.5 * (1.0 + gr * w) / q
        a[s] = 0.5 * gr * w + 0.9189385332046727 - np.log(q)
        s = g <= -32.0
        x = g[s]
        inv = 1.0 / x
        u = inv * inv
        T1 = -1.0 + u * (3.0 + u * (-15.0 + u * (105.0 + u * (-945.0 + u * (10395.0 + u * (-135135.0 + u * 2027025.0))))))
        B1 = 2.0 + u * (-12.0 + u * (90.0 + u * (-840.0 + u * (9450.0 + u * (-124740.0 + u * (1891890.0 + u * -32432400.0))))))
        Tt = 1.0 + u * T1
        da[s] = 0.5 * inv * B1 / (Tt * Tt)
        a[s] = 0.5 * T1 / Tt + 0.9189385332046727 + np.log(-x) - np.log1p(u * T1)
    return a, da


def mes_restated(mu, var, ystar, partials=False):
    """MES(μ, σ²) over arrays μ, σ² for ONE sample vector (and ∂/∂μ, ∂/∂σ²); γ is formed in fp64 and the sum runs in the order
    s = 0 … S − 1, as on the device"""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    ys = np.asarray(ystar, dtype=np.float64).reshape(-1)
    S = ys.shape[0]
    deg = var <= 1e-12
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        sg = np.sqrt(np.where(deg, 1.0, var))
        f, sa, sb = np.zeros_like(mu), np.zeros_like(mu), np.zeros_like(mu)
        for s in range(S):
            g = (mu - ys[s]) / sg
            a, da = mes_a(g)
            f, sa, sb = f + a, sa + da, sb + da * g
        val, dmu, dvar = f / S, sa / (sg * S), -sb / (2.0 * var * S)
    zero = np.where(np.isnan(mu), np.nan, 0.0)
    val, dmu, dvar = np.where(deg, zero, val), np.where(deg, zero, dmu), np.where(deg, zero, dvar)
    return (val, dmu, dvar) if partials else val


def load_golden():
    """dict of the table's arrays; groups share a sample vector: ystar[goff[g]:goff[g + 1]] for the tuples with grp == g"""
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in ("ystar", "goff", "grp", "mu", "var", "mes", "dmu", "dvar")}


def group_samples(tab, g):
    return tab["ystar"][tab["goff"][g]:tab["goff"][g + 1]]


def over_groups(tab, fn):
    """fn(mu, var, ystar) → 3 arrays, evaluated group by group and scattered back to the table's order"""
    out = [np.empty_like(tab["mu"]) for _ in range(3)]
    for g in range(len(tab["goff"]) - 1):
        s = tab["grp"] == g
        for o, v in zip(out, fn(tab["mu"][s], tab["var"][s], group_samples(tab, g))):
            o[s] = v
    return out


def gamma_extremes(tab):
    """(smallest, largest) γ = (μ − y*_s)/σ per tuple over its samples (NaN for σ² ≤ 1e-12)"""
    lo, hi = np.full_like(tab["mu"], np.nan), np.full_like(tab["mu"], np.nan)
    for g in range(len(tab["goff"]) - 1):
        s = (tab["grp"] == g) & (tab["var"] > 1e-12)
        ys = group_samples(tab, g)
        sg = np.sqrt(tab["var"][s])
        lo[s], hi[s] = (tab["mu"][s] - ys.max()) / sg, (tab["mu"][s] - ys.min()) / sg
    return lo, hi


def value_error(got, ref):
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def partial_error(got, ref, sel):
    """max of |got − ref| / max(|ref|, 1e-280) over sel; an exact 0 in the table (σ² ≤ 1e-12, or a' underflowed) needs |got| ≤ 1e-280"""
    assert np.all(np.isfinite(got))
    zero = ref == 0.0
    assert np.all(np.abs(got[zero]) <= 1e-280)
    s = sel & ~zero
    return float(np.max(np.abs(got[s] - ref[s]) / np.maximum(np.abs(ref[s]), 1e-280)))


def check_tail_partials(tab, dmu, dvar):
    """below γ = −64 (every sample): finite, ∂/∂μ ≤ 0, and ∂/∂σ² with the sign of −γ·a' — negative for γ < 0"""
    lo, hi = gamma_extremes(tab)
    tail = hi < -64.0
    assert np.sum(tail) > 100
    assert np.all(np.isfinite(dmu[tail])) and np.all(np.isfinite(dvar[tail]))
    assert np.all(dmu[tail] < 0.0) and np.all(dvar[tail] < 0.0)
    return tail


def test_header_names_mes_within_abi_7():
    hdr = open(HEADER).read()
    assert re.search(r"\bABO_ACQ_MES\s*=\s*6\b", hdr) and re.search(r"#define ABO_ABI_VERSION 7\b", hdr)
    assert A.ACQ_MES == MES and abo._lib.ABI_VERSION == 7 and abo._lib.lib().abo_abi_version() == 7
    for name in ("abo_score_mes", "abo_acq_mes", "abo_cand_acq_mes", "abo_refine_mes", "abo_optimize_acquisition_mes"):
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, hdr) and name in abo._lib.EXPORTS
        assert getattr(abo._lib.lib(), name)
    for name in ("abo_test_mes_partials", "abo_test_acq_grad_mes"):
        assert name in abo._lib.TEST_EXPORTS


def test_table_covers_what_it_says():
    tab = load_golden()
    assert len(tab["mu"]) > 3000 and os.path.getsize(GOLDEN) < 400_000
    sizes = np.diff(tab["goff"])
    assert {1, 3, 16, 1024} <= set(sizes.tolist())
    lo, hi = gamma_extremes(tab)
    nd = tab["var"] > 1e-12
    single = nd & (sizes[tab["grp"]] == 1)
    assert np.nanmax(hi[single]) >= 40.0 and np.nanmin(lo[single]) <= -1e3
    with np.errstate(over="ignore"):
        assert np.any(np.isinf(lo[single] * lo[single]) & np.isfinite(lo[single]))          # γ² overflows, γ does not
    for seam in SEAMS[:2]:
        v = seam
        for _ in range(3):
            v = np.nextafter(v, -np.inf)
        for _ in range(7):
            assert np.any(single & (lo == v)), v
            v = np.nextafter(v, np.inf)
    for v in (0.0, 2.0 ** -1000, -2.0 ** -1000, 2.0 ** -27, -2.0 ** -27):
        assert np.any(single & (lo == v)), v
    assert np.any(tab["var"] == 1e-12) and np.any(tab["var"] == np.nextafter(1e-12, 1.0)) and np.any(tab["var"] == 0.0)
    assert np.all(tab["mes"][~nd] == 0.0) and np.all(tab["dmu"][~nd] == 0.0) and np.all(tab["dvar"][~nd] == 0.0)
    equal = [g for g in range(len(sizes)) if sizes[g] > 1 and np.all(group_samples(tab, g) == group_samples(tab, g)[0])]
    assert {int(sizes[g]) for g in equal} >= {16, 1024}
    assert np.any(nd & (hi < 0.0) & (sizes[tab["grp"]] > 1))                               # every y* above μ
    assert np.all(tab["mes"] >= 0.0) and np.all(tab["dmu"] <= 0.0)


def test_restatement_agrees_with_the_table():
    tab = load_golden()
    val, dmu, dvar = over_groups(tab, lambda m, v, ys: mes_restated(m, v, ys, partials=True))
    lo, hi = gamma_extremes(tab)
    body = (tab["var"] > 1e-12) & (lo >= -64.0)
    ev, em, es = value_error(val, tab["mes"]), partial_error(dmu, tab["dmu"], body), partial_error(dvar, tab["dvar"], body)
    print(f"restated MES against the table: value {ev:.3e}, d/dmu {em:.3e}, d/dvar {es:.3e} (γ ≥ −64)")
    assert ev <= VALUE_BAR and em <= PARTIAL_BAR and es <= PARTIAL_BAR
    check_tail_partials(tab, dmu, dvar)
    # equal samples: the mean of S equal terms is the term, up to the S − 1 roundings of the running sum
    for g in range(len(tab["goff"]) - 1):
        ys = group_samples(tab, g)
        if len(ys) > 1 and np.all(ys == ys[0]):
            s = tab["grp"] == g
            np.testing.assert_allclose(mes_restated(tab["mu"][s], tab["var"][s], ys), mes_restated(tab["mu"][s], tab["var"][s], ys[:1]),
                                       rtol=len(ys) * 2.0 ** -53, atol=0.0)


def test_restatement_is_nonnegative_and_nonincreasing_in_mu():
    g = np.concatenate([np.linspace(-200.0, 45.0, 49001), -np.logspace(2.3, 300.0, 2000)[::-1], np.logspace(1.7, 300.0, 500)])
    g = np.sort(g)
    a, da = mes_a(g)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(da))
    assert np.all(a >= 0.0) and np.all(da <= 0.0)
    # non-increasing up to the rounding of neighbouring values (a few ulp of a, which is ≤ 700 here)
    assert np.all(np.diff(a) <= 8 * np.finfo(float).eps * np.maximum(1.0, a[:-1]))
    for seam in SEAMS[:2]:                                                    # no jump at a cut point beyond rounding
        lo_a, hi_a = mes_a(np.array([np.nextafter(seam, -np.inf), seam, np.nextafter(seam, np.inf)]))[0][[0, 2]]
        assert abs(lo_a - hi_a) <= 1e-12 * max(1.0, lo_a)
    ys = np.array([-1.0, -0.5, -2.0])
    for var in (1e-11, 1e-4, 0.3, 50.0):
        mu = np.linspace(-3.0, 4.0, 4001)
        v = mes_restated(mu, np.full_like(mu, var), ys)
        assert np.all(v >= 0.0) and np.all(np.diff(v) <= 8 * np.finfo(float).eps * np.maximum(1.0, v[:-1]))
    assert np.all(mes_restated([0.3, np.inf], [1e-12, 0.0], ys) == 0.0)       # degenerate variance; an excluded candidate
    assert np.isnan(mes_restated([np.nan, 0.1, np.nan], [1.0, np.nan, 0.0], ys)).all()


class _Recorder:
    """stands in for the loaded library: records each call's arguments and returns ABO_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


class _Model(abo.HipStandardGP):
    def __init__(self):
        pass

    def _require(self):
        return 0xABC0


def _doubles(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n,)).copy()


def test_python_host_marshals_the_samples(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(abo._lib, "lib", lambda: rec)
    ys = [0.25, -1.5, 3.0]
    acq = abo.MaxValueEntropySearch(ys)
    assert acq.kind == MES and acq.ystar.dtype == np.float64 and not acq.ystar.flags.writeable
    m = _Model()
    assert abo.update(acq, [1.0, 2.0], m) is acq and abo.copy(acq) == acq and abo.copy(acq) is not acq
    Z = np.arange(12.0).reshape(4, 3)
    scores, tv, ti = abo.evaluate(acq, m, Z, k=2, idx_base=7)
    name, a = rec.calls[-1]
    assert name == "abo_acq_mes" and a[0] == 0xABC0 and a[2:5] == (4, 3, abo._lib.HOST)
    assert np.array_equal(_doubles(a[5], 3), ys) and a[6:9] == (3, abo._lib.HOST, 7) and a[10] == 2 and a[13] == abo._lib.HOST
    assert a[9] == scores.ctypes.data and a[11] == tv.ctypes.data and a[12] == ti.ctypes.data
    lower, upper = np.zeros(3), np.ones(3)
    x, f = abo.refine_starts(acq, m, Z, lower, upper)
    name, a = rec.calls[-1]
    assert name == "abo_refine_mes" and a[0] == 0xABC0 and np.array_equal(_doubles(a[1], 3), ys) and a[2] == 3
    assert a[5] == 3 and a[7] == 4 and a[9] == x.ctypes.data and a[10] == f.ctypes.data
    A.acquisition_value_and_grad(acq, m, Z)
    name, a = rec.calls[-1]
    assert name == "abo_test_acq_grad_mes" and np.array_equal(_doubles(a[1], 3), ys) and a[2] == 3 and a[4:6] == (4, 3)
    A.optimize_acquisition_device(acq, m, abo.ContinuousDomain(lower, upper), n_grid=500, n_local=9, seed=11)
    name, a = rec.calls[-1]
    assert name == "abo_optimize_acquisition_mes" and np.array_equal(_doubles(a[1], 3), ys) and a[2] == 3 and a[5:9] == (3, 500, 9, 11)
    assert A._library_refinable(acq, m) and A.flatten_terms(acq, m) is None


def test_python_host_refuses_what_the_library_refuses():
    for bad in ([], np.zeros(1025), [0.0, np.nan], [np.inf]):
        with pytest.raises(ValueError):
            abo.MaxValueEntropySearch(bad)
    acq = abo.MaxValueEntropySearch(np.zeros(1024))
    with pytest.raises(TypeError, match="EnsembleAcquisition"):
        abo.EnsembleAcquisition([1.0, 1.0], [abo.UpperConfidenceBound(2.0), acq])
    with pytest.raises(TypeError):
        acq._p0()

    class Sharded(_Model):
        devices = (0, 1)

    with pytest.raises(TypeError, match="single-device"):
        abo.evaluate(acq, Sharded(), np.zeros((2, 2)))


def test_max_value_samples_forwards_to_argmin(monkeypatch):
    seen = {}

    class Paths:
        def argmin(self, Z, k=1, idx_base=0):
            seen["argmin"] = (Z, k)
            return np.array([[0.5], [-2.0], [1.25]]), np.array([[4], [1], [9]])

    def fake_sample_paths(model, S, R=1024, rng=None):
        seen["paths"] = (model, S, R, rng)
        return Paths()

    monkeypatch.setattr(T, "sample_paths", fake_sample_paths)
    out = abo.max_value_samples("model", "grid", 3, R=64, rng=5)
    assert seen["paths"] == ("model", 3, 64, 5) and seen["argmin"] == ("grid", 1)
    assert out.shape == (3,) and out.flags.c_contiguous and np.array_equal(out, [0.5, -2.0, 1.25])
    for S in (0, 1025):
        with pytest.raises(ValueError):
            abo.max_value_samples("model", "grid", S)


def test_julia_shim_passes_the_header_check():
    from tests.test_julia_shim_cpu import _strip_jl_comments, c_prototypes, jl_matches_c, julia_calls
    protos, calls = c_prototypes(), julia_calls(JULIA)
    code = _strip_jl_comments(open(JULIA).read())
    assert len(re.findall(r"LIBABO\.\w+\(", code)) == len(calls) == 2
    assert {c[0] for c in calls} == {"abo_acq_mes", "abo_optimize_acquisition_mes"}
    for name, types, ret, line in calls:
        want = protos[name]
        assert ret == "Int32" and len(types) == len(want), (name, line)
        for k, (jl, c) in enumerate(zip(types, want)):
            assert jl_matches_c(jl, c), f"{name}: argument {k + 1} is {jl}, the header says {c[0]}{'*' * c[1]}"
    assert re.search(r"struct\s+MaxValueEntropySearch\s*<:\s*AbstractAcquisition", code)
    assert "max_value_samples" in code and "path_argmin(" in code and "k=1" in code
    main = open(os.path.join(ROOT, "integration", "julia", "HipStandardGP.jl")).read()
    assert 'include("MaxValueEntropySearch.jl")' in main
    for helper in set(re.findall(r"(?<![\w.!])(_[a-z][a-z0-9_]*!?)\(", code)):
        assert re.search(r"^\s*(function\s+)?%s\(" % re.escape(helper), main + code, flags=re.M), helper
