"""LogEI (ABO_ACQ_LOGEI = 5) without a GPU: the constants of the boundary, the Python and Julia hosts, the host-side decision of the
pruned top-k selection, and the CPU restatement of LogEI that the GPU tests compare against (tests/test_gpu_logei.py imports it from
here) against the mpmath table tests/golden/logei_kat.npz.

The restatement (NumPy + scipy.special.erfcx) is  LogEI = ½log σ² + log h(z),  h = φ + zΦ,  z = Δ/σ,  Δ = (best_y − ξ) − μ,  and
log max(Δ, 0) for σ² ≤ 1e-12, with log h in three ranges of z (directly for z > −1, through erfcx down to −64, the asymptotic series
of the Mills ratio below)."""
import os
import re

import numpy as np
import pytest
from scipy.special import erfc, erfcx

import abstractbayesopt.jl_amd as abo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "abo_hip.h")
JULIA = os.path.join(ROOT, "integration", "julia", "LogExpectedImprovement.jl")
GOLDEN = os.path.join(ROOT, "tests", "golden", "logei_kat.npz")
EI, UCB, PI, MEAN, GRADNORM, LOGEI = 0, 1, 2, 3, 4, 5

# Bars of the restatement against the table (fp64, correctly rounded libm to a few ulp, u = 2⁻⁵³ = 1.1e-16):
#   value    the rounding of z (Δ, sqrt, quotient: 3u) moves log h by 3u·|z|·Φ/h ≤ 3u(z² + 3) ≤ 6u·|ref| + 9u; −z²/2, the constant and
#            the logs add a few u·|ref|; log1p(z·q) near the −64 seam: 2¹²·6u = 2.7e-12 absolute under |ref| ≈ 2048, 1.3e-15 relative.
#            Together below 2e-15·max(1, |ref|); the bar is 1e-14.
#   partials φ/h = 1/(1 + z·q) loses up to 12 bits at the −64 seam: 2¹²·(erfcx, two products, the sum and the quotient: ≤ 16u)
#            = 7.3e-12 relative; the bar is 1e-10 (relative to |ref|), which also holds for the device (tests/test_gpu_logei.py)
VALUE_BAR, PARTIAL_BAR = 1e-14, 1e-10


def logei_restated(mu, var, xi, best_y, partials=False):
    """LogEI(μ, σ²) (and ∂/∂μ, ∂/∂σ²) in NumPy; the arithmetic of Δ and z is fp64, as on the device"""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    delta = (best_y - xi) - mu
    val, dmu, dvar = np.empty_like(mu), np.zeros_like(mu), np.zeros_like(mu)
    deg = var <= 1e-12
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        val[deg] = np.log(np.maximum(delta[deg], 0.0))
        dmu[deg] = np.where(delta[deg] > 0.0, -1.0 / delta[deg], 0.0)
        sg = np.sqrt(var)
        z = delta / sg
        lh, cdf_h, pdf_h = np.full_like(mu, np.nan), np.full_like(mu, np.nan), np.full_like(mu, np.nan)
        a = ~deg & (z > -1.0)
        za = z[a]
        pdf, cdf = np.exp(-0.5 * za * za) * 0.3989422804014327, 0.5 * erfc(-za * 0.7071067811865476)
        h = pdf + za * cdf
        lh[a], cdf_h[a], pdf_h[a] = np.log(h), cdf / h, pdf / h
        b = ~deg & (z <= -1.0) & (z > -64.0)
        zb = z[b]
        q = 1.2533141373155003 * erfcx(-zb * 0.7071067811865476)              # Φ/φ
        lh[b] = -0.5 * zb * zb - 0.9189385332046727 + np.log1p(zb * q)
        pdf_h[b] = 1.0 / (1.0 + zb * q)
        cdf_h[b] = q * pdf_h[b]
        c = ~deg & (z <= -64.0)
        zc = z[c]
        u = 1.0 / (zc * zc)
        S = u * (-3.0 + u * (15.0 + u * (-105.0 + u * 945.0)))
        T = 1.0 + u * (-1.0 + u * (3.0 + u * (-15.0 + u * 105.0)))
        lh[c] = -0.5 * zc * zc - 0.9189385332046727 - 2.0 * np.log(-zc) + np.log1p(S)
        pdf_h[c] = zc * zc / (1.0 + S)
        cdf_h[c] = -zc * T / (1.0 + S)
        nd = ~deg
        val[nd] = 0.5 * np.log(var[nd]) + lh[nd]
        dmu[nd] = -cdf_h[nd] / sg[nd]
        dvar[nd] = 0.5 * pdf_h[nd] / var[nd]
    return (val, dmu, dvar) if partials else val


def load_golden():
    """(μ, σ², ξ, best_y, LogEI, ∂/∂μ, ∂/∂σ²) as arrays over the table's tuples"""
    with np.load(GOLDEN) as g:
        return tuple(g[k] for k in ("mu", "var", "xi", "best_y", "logei", "dmu", "dvar"))


def value_error(got, ref):
    """max of |got − ref| / max(1, |ref|) over the finite reference values; −Inf must be matched exactly"""
    inf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), inf), "−Inf where the table has a finite value, or the other way round"
    assert np.all(np.isfinite(got[~inf]))
    return float(np.max(np.abs(got[~inf] - ref[~inf]) / np.maximum(1.0, np.abs(ref[~inf]))))


def partial_error(got, ref):
    """max of |got − ref| / max(|ref|, 1e-280); an exact 0 in the table (the σ² ≤ 1e-12 branch) must be matched exactly.  The floor:
    ∂/∂σ² = φ/(2σ²h) leaves the normal range with φ from z ≈ 38.5 up, where fp64 keeps no relative precision (a subnormal φ times
    1/(2σ²h) ≤ 1e11/76 stays below 1e-296)"""
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0)
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.maximum(np.abs(ref[~zero]), 1e-280)))


def _by_pair(f, mu, var, xi, best):
    out = [np.empty_like(mu) for _ in range(3)]
    for x, b in sorted(set(zip(xi, best))):
        s = (xi == x) & (best == b)
        for o, v in zip(out, f(mu[s], var[s], float(x), float(b))):
            o[s] = v
    return out


def test_header_defines_logei_within_abi_7():
    hdr = open(HEADER).read()
    assert re.search(r"\bABO_ACQ_LOGEI\s*=\s*5\b", hdr)
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr)
    assert abo._lib.ABI_VERSION == 7 and abo._lib.lib().abo_abi_version() == 7
    assert re.search(r"\bABO_ACQ_GRADNORM_UCB\s*=\s*4\b", hdr) and re.search(r"\bABO_ACQ_EI\s*=\s*0\b", hdr)


def test_python_host_has_the_class():
    from abstractbayesopt.jl_amd import acquisition as A
    assert A.ACQ_LOGEI == LOGEI
    a = abo.LogExpectedImprovement(0.01, 10.0)
    assert a.kind == LOGEI and a._p0() == 0.01 and a._best() == 10.0
    gp = abo.HipStandardGP(abo.Matern52Kernel(), 1e-3)
    b = abo.update(a, [2.0, 1.0, 0.5], gp)
    assert isinstance(b, abo.LogExpectedImprovement) and b.best_y == 0.5 and b.xi == 0.01
    assert abo.copy(a) == a and abo.copy(a) is not a
    assert not isinstance(a, abo.ExpectedImprovement)                    # q-EI and other EI-only paths do not take it for EI
    # a term of a weighted-sum objective, plain and inside an ensemble
    assert A.flatten_terms(a) == [(LOGEI, 0.01, 10.0, 1.0)]
    ens = abo.EnsembleAcquisition([1.0, 1.0], [a, abo.UpperConfidenceBound(2.0)])
    assert A.flatten_terms(ens) == [(LOGEI, 0.01, 10.0, 0.5), (UCB, 2.0, 0.0, 0.5)]
    upd = abo.update(ens, [3.0, -1.0], gp)
    assert upd.acquisitions[0] == abo.LogExpectedImprovement(0.01, -1.0)


def _plan(rows, M, k, want_scores=0, kind=EI, p0=0.01, p_out=1, int8=1, d=8):
    out = np.zeros(4, dtype=np.int64)
    abo._lib.check(abo._lib.lib().abo_test_prune_plan(rows, M, k, want_scores, kind, p0, p_out, int8, d, out.ctypes.data))
    return [int(v) for v in out]


def test_pruned_selection_takes_logei_under_eis_conditions():
    base = dict(rows=8192, M=1 << 20, k=100)
    assert _plan(**base, kind=LOGEI)[0] == 1
    variants = [dict(), dict(want_scores=1), dict(k=0), dict(p_out=9), dict(int8=0), dict(rows=256), dict(rows=257), dict(M=4095),
                dict(M=4096), dict(k=1000, M=15999), dict(k=1000, M=16000), dict(p0=-1.0), dict(d=4096)]
    for v in variants:
        assert _plan(**{**base, **v, "kind": LOGEI}) == _plan(**{**base, **v, "kind": EI}), v
    assert _plan(**base, kind=PI)[0] == 0 and _plan(**base, kind=MEAN)[0] == 0 and _plan(**base, kind=GRADNORM)[0] == 0


def test_julia_shim_defines_the_type():
    src = open(JULIA).read()
    code = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    assert re.search(r"struct\s+LogExpectedImprovement(\{\w+\})?\s*<:\s*AbstractAcquisition", code)
    m = re.search(r"_acq_args\(a::LogExpectedImprovement\)\s*=\s*\(Int32\((\d+)\)", code)
    assert m and int(m.group(1)) == LOGEI
    assert re.search(r"\(a::LogExpectedImprovement\)\(m::HipStandardGP, x::AbstractVector\)\s*=\s*_acq\(m, x, _acq_args\(a\)\.\.\.\)\[1\]", code)
    assert re.search(r"^update\(a::LogExpectedImprovement,", code, flags=re.M) and "Base.copy(a::LogExpectedImprovement)" in code
    assert "ccall" not in code and "LIBABO" not in code                  # no call of its own: it rides on HipStandardGP.jl's helpers
    main = open(os.path.join(ROOT, "integration", "julia", "HipStandardGP.jl")).read()
    assert 'include("LogExpectedImprovement.jl")' in main
    for helper in set(re.findall(r"(?<![\w.!])(_[a-z][a-z0-9_]*!?)\(", code)) - {"_get_minimum"}:
        assert re.search(r"^\s*(function\s+)?%s\(" % re.escape(helper), main + code, flags=re.M), helper


def test_restatement_agrees_with_the_table():
    mu, var, xi, best, ref, rdmu, rdvar = load_golden()
    assert len(mu) > 6000 and np.sum(np.isneginf(ref)) >= 40
    val, dmu, dvar = _by_pair(lambda m, v, x, b: logei_restated(m, v, x, b, partials=True), mu, var, xi, best)
    ev, em, es = value_error(val, ref), partial_error(dmu, rdmu), partial_error(dvar, rdvar)
    print(f"restated LogEI against the table: value {ev:.3e}, d/dmu {em:.3e}, d/dvar {es:.3e}")
    assert ev <= VALUE_BAR and em <= PARTIAL_BAR and es <= PARTIAL_BAR
    # the table covers what it says: all three ranges, both seams to the ulp, z = 0, the degenerate branch on both sides of 1e-12
    z = ((best - xi) - mu) / np.sqrt(np.where(var > 0, var, 1.0))
    nd = var > 1e-12
    for s in (-1.0, -64.0):
        for v in (np.nextafter(s, -np.inf), s, np.nextafter(s, 0.0)):
            assert np.any(nd & (z == v)), v
    assert np.any(nd & (z == 0.0)) and np.min(z[nd]) <= -9.9e7 and np.max(z[nd]) >= 39.9
    assert np.any(var == 1e-12) and np.any(var == np.nextafter(1e-12, 1.0))
    assert np.min(var[nd]) <= 1e-11 and np.max(var) >= 1e4
    # where EI is representable, exp(LogEI) is EI
    from oracle import gp_oracle as O
    for x, b in sorted(set(zip(xi, best))):
        s = (xi == x) & (best == b)
        ei = O.expected_improvement(mu[s], var[s], float(b), float(x))
        ok = ei >= 1e-300
        assert np.max(np.abs(np.exp(ref[s][ok]) / ei[ok] - 1.0)) <= 1e-9
