"""The fp32 tail of the first bound level (csrc/kgen_tail32.hip, csrc/abo_kappa.h: kappa_tail32), restated in NumPy
float32 and held against the fp64 oracle: the constants the guard is built from — read from abo_kappa.h — must bound what the
sequence does, with the two transcendental instructions pushed to the 1 ulp the ISA allows them in either direction.

  * κ's sensitivity figures (TAIL32_REL_R, TAIL32_LIP_R) against the oracle's κ on a dense grid;
  * |kappa_tail32(q) − κ(√q)| ≤ TAIL32_ETA_EVAL for fp32 q: 0, denormal, tiny, random, large, at and beyond the clamp of the exponent;
  * the pair formula η = ETA + REL_R·(dp/2 + 1)·v₁ + LIP_R·(v₁·√(2w) + R_ABS) against fp64 inputs rounded to fp32, difference form,
    fp32 fma chain: candidates in the box, ON a training point, 1e-12 from one, +1000 per coordinate; every padded dimension;
  * the sum formula ε on a small problem with α of mixed signs and L1 norm 10⁵ (the fp64 accumulation of the fp32 values)."""
import os
import re

import numpy as np
import pytest

from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
V = 2.0 ** -24
U = 2.0 ** -53
V1 = V * (1.0 + 2.0 ** -10)
FAMILIES = [O.SE, O.MATERN52, O.MATERN72, O.MATERN32]


def header_constants():
    """the constexpr values of csrc/abo_kappa.h by name"""
    with open(os.path.join(ROOT, "abstractbayesopt.jl_amd", "csrc", "abo_kappa.h"), encoding="utf-8") as f:
        src = f.read()
    out = {}
    for name, val in re.findall(r"constexpr (?:double|float) (TAIL\w+) = ([^;]+);", src):
        val = val.strip().rstrip("f")
        out[name] = float.fromhex(val) if "0x" in val else float(val)
    return out


C = header_constants()


def test_constants_are_read():
    assert C["TAIL32_ETA_EVAL"] == 2.0 ** -20 and C["TAIL32_REL_R"] == 0.74 and C["TAIL32_LIP_R"] == 0.64
    assert C["TAIL32_R_ABS"] == 2.0 ** -59 and C["TAIL32_T_MIN"] == -150.0 and C["TAIL_W_MAX"] == 2.0 ** 40


def fma32(a, b, c):
    """fl32(a·b + c): the product of two fp32 numbers is exact in fp64; the sum's fp64 rounding ahead of the fp32 one moves the result
    by at most 2⁻²⁹ of an fp32 ulp more than one rounding would"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def ulp_shift(x, k):
    """x moved by k fp32 ulps (k in {−1, 0, 1}); zeros, infinities and NaN stay"""
    x = np.asarray(x, F32)
    if k == 0:
        return x
    y = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf))
    return np.where((x == 0) | ~np.isfinite(x), x, y).astype(F32)


def flush(x):
    """what v_sqrt_f32 and v_exp_f32 do with a denormal input or result"""
    x = np.asarray(x, F32)
    return np.where(np.abs(x) < F32(2.0 ** -126), F32(0.0) * x, x).astype(F32)


def kappa_tail32(family, q, ks=0, ke=0):
    """kappa_tail32<family> of abo_kappa.h on an fp32 array; the sqrt and the exp results moved by ks and ke ulps"""
    q = np.asarray(q, F32)
    l2e = 1.44269504088896340736
    one = np.ones_like(q)

    def exp2c(t):
        with np.errstate(under="ignore"):
            return flush(ulp_shift(flush(np.exp2(np.maximum(flush(t), F32(C["TAIL32_T_MIN"])))), ke))

    if family == O.SE:
        return exp2c(q * F32(-0.5 * l2e))
    with np.errstate(invalid="ignore"):
        d = ulp_shift(np.sqrt(flush(q)), ks)
    if family == O.MATERN52:
        s = 2.23606797749978969640917366873128
        p = fma32(q, np.full_like(q, F32(5.0 / 3.0)), fma32(d, np.full_like(q, F32(s)), one))
    elif family == O.MATERN72:
        s = 2.64575131106459059050161575363926
        p = fma32(q * d, np.full_like(q, F32(7.0 * s / 15.0)),
                  fma32(q, np.full_like(q, F32(14.0 / 5.0)), fma32(d, np.full_like(q, F32(s)), one)))
    else:
        s = 1.73205080756887729352744634150587
        p = fma32(d, np.full_like(q, F32(s)), one)
    with np.errstate(over="ignore", invalid="ignore"):
        return (p * exp2c(d * F32(-s * l2e))).astype(F32)


def kappa_of_r(family, r):
    return O.kappa(family, np.asarray(r, np.float64) ** 2)


@pytest.mark.parametrize("family", FAMILIES)
def test_sensitivity_figures(family):
    r = np.concatenate([np.linspace(0.0, 12.0, 1200001), 10.0 ** np.linspace(-12, 3, 20001)])
    r.sort()
    h = 1e-7
    dk = np.abs(kappa_of_r(family, r + h) - kappa_of_r(family, np.maximum(r - h, 0.0))) / (r + h - np.maximum(r - h, 0.0))
    lip, rel = dk.max(), (r * dk).max()
    print(f"family {family}: max |dκ/dr| = {lip:.4f} (stated {C['TAIL32_LIP_R']}), max |r·dκ/dr| = {rel:.4f} (stated {C['TAIL32_REL_R']})")
    assert lip <= C["TAIL32_LIP_R"] - 1e-3 and rel <= C["TAIL32_REL_R"] - 1e-3


def _grid_q():
    rng = np.random.default_rng(32)
    t_edge = []
    for s in (0.5, 3.0 ** 0.5, 5.0 ** 0.5, 7.0 ** 0.5):          # where the scaled exponent crosses −126 (flush) and −150 (clamp)
        for t in (-125.0, -126.0, -127.0, -140.0, -149.0, -150.0, -151.0, -200.0):
            a = -t / 1.44269504088896340736
            t_edge += [(a / s) ** 2, a * 2.0]
    fixed = [0.0, 1e-45, 1e-40, 2.0 ** -126, 1e-30, 1e-24, 1e-13, 1e-12, 1e-10, 1e-6, 0.5, 1.0, 2.0, 100.0, 1e3, 1e5, 1e6, 1e9, 1e12, 2.0 ** 41]
    q = np.concatenate([fixed, t_edge, 10.0 ** rng.uniform(-8, 3, 200000), rng.uniform(0, 50, 200000), rng.uniform(0, 4, 100000)])
    return q.astype(F32)                                         # fp32 numbers: what the kernel hands over


@pytest.mark.parametrize("family", FAMILIES)
def test_evaluation_within_eta_eval(family):
    q = _grid_q()
    ref = O.kappa(family, q.astype(np.float64))
    worst = 0.0
    for ks in (-1, 0, 1):
        for ke in (-1, 0, 1):
            got = kappa_tail32(family, q, ks, ke).astype(np.float64)
            assert np.all(np.isfinite(got))
            err = np.abs(got - ref)
            worst = max(worst, err.max())
            assert np.all(err <= C["TAIL32_ETA_EVAL"]), (ks, ke, q[np.argmax(err)], err.max())
    print(f"family {family}: max |kappa_tail32 - kappa| = {worst:.3e} = {worst / V:.2f} v (stated {C['TAIL32_ETA_EVAL']:.3e} = 16 v)")
    # at and beyond the clamp the value is 0 on both sides
    big = q[q.astype(np.float64) >= 2.0e4]
    assert big.size and np.all(kappa_tail32(family, big) == 0.0)
    assert kappa_tail32(family, np.zeros(1, F32))[0] == 1.0


def pair_r2(x, z):
    """the kernel's fp32 squared distances: x [n, dp], z [m, dp] fp64 → [m, n] fp32, difference form, fma chain from 0"""
    xs, zs = x.astype(F32), z.astype(F32)
    r = np.zeros((z.shape[0], x.shape[0]), F32)
    for c in range(x.shape[1]):
        e = (xs[None, :, c] - zs[:, None, c]).astype(F32)
        r = fma32(e, e, r)
    return r


def eta_pair(dp, w):
    return C["TAIL32_ETA_EVAL"] + C["TAIL32_REL_R"] * (0.5 * dp + 1.0) * V1 + C["TAIL32_LIP_R"] * (V1 * np.sqrt(2.0 * w) + C["TAIL32_R_ABS"])


def _points(d, dp, n, m, rng):
    x = np.zeros((n, dp))
    z = np.zeros((m, dp))
    x[:, :d] = rng.uniform(0.0, 1.0, (n, d)) * rng.choice([0.3, 1.0, 3.0])
    z[:, :d] = rng.uniform(0.0, 1.0, (m, d)) * rng.choice([0.3, 1.0, 3.0])
    z[0] = x[3]                                                   # on a training point
    z[1, :d] = x[5, :d] + 1e-12                                   # 1e-12 from one: the rounding of the inputs is all there is
    z[2, :d] = x[7, :d] * (1.0 + 2.0 ** -25)                      # half an fp32 ulp away
    z[3:7, :d] += 1000.0                                          # far: exponent beyond the clamp, a large w
    z[7, :d] = 1e-30                                              # squares underflow in fp32
    return x, z


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d,dp", [(1, 1), (2, 2), (3, 4), (5, 8), (8, 8), (16, 16), (32, 32)])
def test_pair_error_within_eta(family, d, dp):
    rng = np.random.default_rng(1000 * family + d)
    x, z = _points(d, dp, 400, 300, rng)
    w = np.max(np.sum(x * x, axis=1)) + np.sum(z * z, axis=1)
    assert np.all(w < C["TAIL_W_MAX"])
    r2 = ((x[None, :, :] - z[:, None, :]) ** 2).sum(axis=2)       # fp64: the exact distance to 1e-16 relative
    r2[0, 3] = 0.0
    ref = O.kappa(family, r2)
    q = pair_r2(x, z)
    eta = eta_pair(dp, w)[:, None]
    worst = 0.0
    for ks, ke in ((0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1)):
        err = np.abs(kappa_tail32(family, q, ks, ke).astype(np.float64) - ref)
        worst = max(worst, np.max(err / eta))
        assert np.all(err <= eta), (ks, ke, np.unravel_index(np.argmax(err / eta), err.shape), err.max())
    print(f"family {family} d={d} dp={dp}: max err/eta = {worst:.3f}, eta in [{eta.min():.3e}, {eta.max():.3e}]")
    assert eta_pair(8, 16.0) < 1.4e-6                             # the benchmark's shape: the figure DESIGN quotes


@pytest.mark.parametrize("family", FAMILIES)
def test_sum_error_within_eps(family):
    """μ̃_tail as the kernel sums it (fp64 products of the fp32 values with fl(σ_f²·α_k), fp64 additions) against the fp64 sum, α of
    mixed signs with ‖α‖₁ ≈ 10⁵; the head is empty, so the full launch's own terms of ε are not exercised, only left in"""
    rng = np.random.default_rng(7 + family)
    d, dp, n, m, sf2, mean_c = 8, 8, 2000, 256, 1.3, 0.2
    x, z = _points(d, dp, n, m, rng)
    alpha = rng.standard_normal(n) * (1e5 / n) * 1.25
    a_tail = a_all = float(np.sum(np.abs(alpha)))
    w = np.max(np.sum(x * x, axis=1)) + np.sum(z * z, axis=1)
    r2 = ((x[None, :, :] - z[:, None, :]) ** 2).sum(axis=2)
    mu = sf2 * (O.kappa(family, r2) @ alpha)
    kv = kappa_tail32(family, pair_r2(x, z), 1, -1).astype(np.float64)
    mu_t = np.zeros(m)
    for k in range(n):                                            # one fma per pair, in the sweep's order
        mu_t = mu_t + kv[:, k] * (alpha[k] * sf2)
    eps = 1.0001 * sf2 * ((eta_pair(dp, w) + (dp + 14) * U) * a_tail + (2.0 * n + 64.0) * U * a_all) + 8.0 * U * abs(mean_c)
    err = np.abs(mu_t - mu)
    print(f"family {family}: ‖α‖₁ = {a_all:.3e}, max err = {err.max():.3e}, eps in [{eps.min():.3e}, {eps.max():.3e}], max err/eps = {np.max(err / eps):.3f}")
    assert np.all(err <= eps)
