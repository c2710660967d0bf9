"""Writes tests/golden/mes_kat.npz: max-value entropy search (ABO_ACQ_MES) and its partial derivatives ∂/∂μ, ∂/∂σ² from mpmath at 60
digits and more, rounded to the nearest double, for ≈ 3 200 tuples (μ, σ², y*[S]).

    MES = (1/S)·Σ_s a(γ_s),  γ_s = (μ − y*_s)/σ,  a(γ) = γ·φ(γ)/(2Φ(γ)) − log Φ(γ)                for σ² > 1e-12
    MES = 0, ∂/∂μ = ∂/∂σ² = 0                                                                       for σ² ≤ 1e-12
    ∂/∂μ = (1/S)·Σ a'(γ_s)/σ,  ∂/∂σ² = −(1/S)·Σ a'(γ_s)·γ_s/(2σ²),  a'(γ) = −(r/2)·(1 + γ² + γ·r),  r = φ/Φ

The reference is evaluated EXACTLY at the stored doubles (γ formed in extended precision).  γ·r/2 and −log Φ cancel like γ²/2 against
a result of size log|γ|, and the bracket of a' cancels twice over, so the working precision grows with |γ|: 60 + 4·log₁₀|γ| digits.
Below γ = −10⁴ the converged asymptotic series takes over (tail_series); log Φ is log1p(−Φ(−γ)) for γ > 0.

The table is stored by GROUPS that share one sample vector (the GPU test scores a group per call): `ystar` holds the vectors back to
back, `goff[g] … goff[g+1]` is group g's slice, `grp[i]` the group of tuple i.  The groups:
    S = 1   y* ∈ {0, −1.25, 0.75}: γ on a grid over [−80, 40] (step 0.05), γ = −10^[0, 8], γ = ±10^{10 … 300} (γ² overflows beyond
            1.3·10¹⁵⁴), the seams of the evaluation's ranges (−32, −1 each −3 … +3 ulps, 0 and ±2⁻²⁷, ±2⁻³⁰⁰, ±2⁻¹⁰⁰⁰) at σ ∈ {½, 1, 2} with y* = 0 (so that the
            fp64 quotient is that γ exactly), σ² on both sides of 1e-12 with μ above, at and below y*
    S = 3, 16   random sample vectors around a random centre, μ swept from far below the samples (a y* above μ: γ < 0) to far above
    S = 16  equal samples
    S = 1024  a spread vector (γ from −10³ to 40 within one sum), equal samples, all samples above μ, a typical draw
σ² cycles through 1e-11 … 1e4.

Run from the repository root:  python tests/golden/make_mes_golden.py      (needs mpmath; the tests only read the file)"""
import os

import mpmath as mp
import numpy as np

VARS = [10.0 ** e for e in range(-11, 5)]
SEAMS = (-32.0, -1.0, 0.0)


def tail_series(g):
    """γ < −10⁴, where mpmath's erfc gives up: the asymptotic series of the Mills ratio Φ/φ = T(u)/|γ|, u = 1/γ², T = Σ c_k u^k,
    c_k = (−1)^k (2k−1)!!, summed to 70 digits (terms fall by 10⁻⁸·(2k+1) each: 12 of them), and the two combinations that cancel
    written without a subtraction:  T = 1 + u·T₁,  a = T₁/(2T) + ½log 2π + log|γ| − log T,  bracket = u·B₁/T with
    B₁ = Σ (c_{j+1} + c_{j+2}) u^j,  a' = B₁/(2γT²).  Checked against the erfc route where both run (main: γ = −10³)."""
    with mp.workdps(80):
        x, u = -g, 1 / (g * g)
        c = [mp.mpf(1)]
        for k in range(1, 16):
            c.append(-c[-1] * (2 * k - 1))
        T1 = sum(c[k + 1] * u ** k for k in range(14))
        B1 = sum((c[j + 1] + c[j + 2]) * u ** j for j in range(14))
        T = 1 + u * T1
        return T1 / (2 * T) + mp.log(2 * mp.pi) / 2 + mp.log(x) - mp.log(T), B1 / (2 * g * T * T)


def a_and_da(g):
    """(a(γ), a'(γ)) as mpf at a working precision that covers the cancellation"""
    if g > 1e4:                       # a < 10^(−10⁷): 0 in any double (mpmath's erfc does not take arguments this large)
        return mp.mpf(0), mp.mpf(0)
    if g < -1e4:
        return tail_series(g)
    dps = 60 + (int(4 * mp.log10(abs(g))) if abs(g) > 1 else 0)
    with mp.workdps(dps):
        pdf = mp.npdf(g)
        if g > 0:
            tail = mp.ncdf(-g)
            cdf, logcdf = 1 - tail, mp.log1p(-tail)
        else:
            cdf = mp.ncdf(g)
            logcdf = mp.log(cdf)
        r = pdf / cdf
        return g * r / 2 - logcdf, -(r / 2) * (1 + g * g + g * r)


def reference(mu, var, ys):
    """(MES, ∂/∂μ, ∂/∂σ²) at the doubles given, as doubles"""
    if var <= 1e-12:
        return 0.0, 0.0, 0.0
    mp.mp.dps = 60
    mu_, var_ = mp.mpf(float(mu)), mp.mpf(float(var))
    sg = mp.sqrt(var_)
    f = dm = dv = mp.mpf(0)
    for y in ys:
        g = (mu_ - mp.mpf(float(y))) / sg
        a, da = a_and_da(g)
        f += a
        dm += da
        dv += da * g
    n = len(ys)
    return float(f / n), float(dm / (sg * n)), float(-dv / (2 * var_ * n))


def groups():
    """[(ystar, [(μ, σ²), …]), …]"""
    rng = np.random.default_rng(20171)
    out = []
    n = 0
    singles = {0.0: [], -1.25: [], 0.75: []}
    keys = list(singles)

    def at_gamma(g, var, y):
        singles[y].append((float(y + g * np.sqrt(var)), float(var)))

    for g in np.linspace(-80.0, 40.0, 2401):
        at_gamma(g, VARS[n % 16], keys[n % 3])
        n += 1
    for g in -np.logspace(0.0, 8.0, 200):
        at_gamma(g, VARS[n % 16], keys[n % 3])
        n += 1
    for e in (10, 50, 100, 153, 154, 155, 160, 200, 300):
        for sign in (-1.0, 1.0):
            for lead in (1.0, 1.5):
                at_gamma(sign * lead * 10.0 ** e, VARS[n % 4], 0.0)          # σ ≤ 1e-4: μ = γσ stays finite
                n += 1
    for seam in SEAMS:
        steps = [seam]
        lo = hi = seam
        for _ in range(3):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            steps += [lo, hi]
        if seam == 0.0:                                                      # (its neighbours in ulps are subnormal: powers of two instead)
            steps = [0.0, -2.0 ** -1000, 2.0 ** -1000, -2.0 ** -300, 2.0 ** -300, -2.0 ** -27, 2.0 ** -27]
        for g in steps:
            for sg in (0.5, 1.0, 2.0):
                mu = g * sg                                                  # exact: the device's μ/σ is g
                assert mu / sg == g
                singles[0.0].append((float(mu), sg * sg))
    for var in (0.0, 1e-18, 1e-13, 1e-12, float(np.nextafter(1e-12, 1.0))):
        for y in keys:
            for delta in (3.0, 0.125, 1e-7, 0.0, -1e-7, -2.0):
                singles[y].append((float(y + delta), var))
    for y in keys:
        out.append((np.array([y]), singles[y]))

    def sweep(ys, count):
        """μ from far below the samples to far above, in units of σ"""
        pts = []
        for i, t in enumerate(np.linspace(-1.0, 1.0, count)):
            var = VARS[(i * 7 + len(out)) % 16]
            g = np.sign(t) * (10.0 ** (abs(t) * 2.2) - 1.0) * (-1.0 if i % 5 == 0 else 1.0)          # |γ| up to ≈ 157, both signs
            pts.append((float(np.mean(ys) + g * np.sqrt(var)), float(var)))
        return pts

    for S, ng, count in ((3, 6, 40), (16, 4, 30)):
        for _ in range(ng):
            centre, spread = rng.normal(0.0, 2.0), 10.0 ** rng.uniform(-3.0, 0.5)
            ys = centre + spread * rng.standard_normal(S)
            out.append((ys, sweep(ys, count)))
    out.append((np.full(16, -0.4375), sweep(np.full(16, -0.4375), 30)))
    big = 1024
    spread = np.concatenate([-np.linspace(-40.0, 0.0, big // 2), np.logspace(0.0, 3.0, big // 2)])    # μ = 0, σ = 1: γ = −y*
    out.append((spread, [(0.0, 1.0), (0.5, 4.0), (-3.0, 0.01)]))
    out.append((np.full(big, 1.5), [(1.0, 1.0), (2.5, 0.25), (40.0, 1.0)]))
    above = 5.0 + np.abs(rng.standard_normal(big))
    out.append((above, [(0.0, 1.0), (-20.0, 1e-3), (4.9, 1e-8)]))
    typical = -2.0 + 0.1 * rng.standard_normal(big)
    out.append((typical, [(0.0, 1.0), (-1.9, 0.04), (-2.3, 1e-4), (3.0, 1e-11)]))
    return out


def main():
    with mp.workdps(200):               # the series against the erfc route at γ = −10³ (u = 10⁻⁶: the 14 terms reach 10⁻⁷⁰)
        g = mp.mpf(-1000)
        r = mp.npdf(g) / mp.ncdf(g)
        for got, want in zip(tail_series(g), (g * r / 2 - mp.log(mp.ncdf(g)), -(r / 2) * (1 + g * g + g * r))):
            assert abs(got / want - 1) < mp.mpf(10) ** -60
    ystar, goff, grp, rows = [], [0], [], []
    for g, (ys, pts) in enumerate(groups()):
        ys = np.asarray(ys, dtype=np.float64)
        ystar.append(ys)
        goff.append(goff[-1] + len(ys))
        for mu, var in pts:
            grp.append(g)
            rows.append([mu, var, *reference(mu, var, ys)])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mes_kat.npz")
    c = np.array(rows, dtype=np.float64)            # binary: every double exactly
    np.savez_compressed(path, ystar=np.concatenate(ystar), goff=np.array(goff, dtype=np.int64), grp=np.array(grp, dtype=np.int32),
                        mu=c[:, 0], var=c[:, 1], mes=c[:, 2], dmu=c[:, 3], dvar=c[:, 4])
    print(len(rows), "tuples in", len(goff) - 1, "groups,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
