"""Writes tests/golden/logei_kat.npz: LogEI and its partial derivatives ∂/∂μ, ∂/∂σ² from mpmath at 80 digits, rounded to the
nearest double, for ≈ 6 000 tuples (μ, σ², ξ, best_y).

    LogEI = log σ + log h(z),  h(z) = φ(z) + z·Φ(z),  z = Δ/σ,  Δ = (best_y − ξ) − μ          for σ² > 1e-12
    LogEI = log max(Δ, 0)  (−Inf for Δ ≤ 0),  ∂/∂μ = −1/Δ for Δ > 0 else 0,  ∂/∂σ² = 0          for σ² ≤ 1e-12
    ∂/∂μ = −Φ(z)/(σ·h(z)),  ∂/∂σ² = φ(z)/(2σ²·h(z))

The reference is evaluated EXACTLY at the stored doubles (Δ and z formed in 80 digits), so a tuple tests the epilogue's arithmetic,
rounding of Δ and z included.  ξ and best_y are dyadic rationals: best_y − ξ is then exact in fp64 and Δ = (best_y − ξ) − μ is one
rounding of an exact difference — with a rounded best_y − ξ the value of LogEI near z = 0 at σ ≈ 1e-5 would move by 1e-11 for a
reason that is the input's conditioning, not the epilogue's.

The tuples: z on a grid over [−80, 40] (step 0.025) and on a coarser one (step 0.25) at two more variances each; z = −10^[0, 8];
the seams of the three evaluation ranges, z = −1 and z = −64, each ± 1 ulp, at σ ∈ {½, 1, 2} (only tuples whose fp64 Δ/σ is that z exactly); z = 0;
σ² = 1e-12 and the next double above it (and three variances below) with Δ > 0, = 0, < 0.  σ² cycles through 1e-11 … 1e4.

Run from the repository root:  python tests/golden/make_logei_golden.py      (needs mpmath; the tests only read the file)"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 80
PAIRS = [(0.0, 0.0), (0.015625, -1.25), (0.5, 0.75), (0.0, -2.0)]           # (ξ, best_y)
VARS = [10.0 ** e for e in range(-11, 5)]


def reference(mu, var, xi, best):
    """(LogEI, ∂/∂μ, ∂/∂σ²) at the doubles given, as doubles"""
    mu, var, xi, best = (mp.mpf(float(v)) for v in (mu, var, xi, best))
    delta = (best - xi) - mu
    if var <= mp.mpf(1e-12):
        if delta > 0:
            return float(mp.log(delta)), float(-1 / delta), 0.0
        return float("-inf"), 0.0, 0.0
    sg = mp.sqrt(var)
    z = delta / sg
    pdf = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)
    cdf = mp.erfc(-z / mp.sqrt(2)) / 2
    h = pdf + z * cdf
    return float(mp.log(sg) + mp.log(h)), float(-cdf / (sg * h)), float(pdf / (2 * var * h))


def tuples():
    out = []

    def at_z(z, var, pair):
        xi, best = PAIRS[pair]
        out.append((pair, float((best - xi) - z * np.sqrt(var)), float(var)))

    n = 0
    for z in np.linspace(-80.0, 40.0, 4801):
        at_z(z, VARS[n % 16], n % 4)
        n += 1
    for z in np.linspace(-80.0, 40.0, 481):
        at_z(z, VARS[(n + 5) % 16], (n + 1) % 4)
        at_z(z, VARS[(n + 11) % 16], (n + 2) % 4)
        n += 1
    for z in -np.logspace(0.0, 8.0, 400):
        at_z(z, VARS[n % 16], n % 4)
        n += 1
    for seam in (-1.0, -64.0):
        for z in (np.nextafter(seam, -np.inf), seam, np.nextafter(seam, 0.0)):
            for sg in (0.5, 1.0, 2.0):
                for pair in range(4):
                    xi, best = PAIRS[pair]
                    mu = (best - xi) - z * sg            # kept where the device's own Δ/σ lands on z exactly (always for best − ξ = 0)
                    if ((best - xi) - mu) / sg == z:
                        out.append((pair, float(mu), sg * sg))
                    else:
                        assert pair != 0
    for var in VARS:
        for pair in range(4):
            at_z(0.0, var, pair)
    for var in (0.0, 1e-18, 1e-13, 1e-12, float(np.nextafter(1e-12, 1.0))):
        for pair in range(4):
            xi, best = PAIRS[pair]
            for delta in (3.0, 0.125, 1e-7, 0.0, -1e-7, -2.0):
                out.append((pair, float((best - xi) - delta), var))
    return out


def main():
    rows = []
    for pair, mu, var in tuples():
        xi, best = PAIRS[pair]
        rows.append([xi, best, mu, var, *reference(mu, var, xi, best)])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "logei_kat.npz")
    c = np.array(rows, dtype=np.float64)            # binary: every double exactly, a third of the size of a decimal table
    np.savez_compressed(path, xi=c[:, 0], best_y=c[:, 1], mu=c[:, 2], var=c[:, 3], logei=c[:, 4], dmu=c[:, 5], dvar=c[:, 6])
    print(len(rows), "tuples,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
