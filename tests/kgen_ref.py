"""Reference of the kernel-matrix generators (csrc/kgen_core.h, kgen_grad_core.h, kgen.hip) — NumPy, no GPU.  TEST INFRASTRUCTURE ONLY.

Exact inputs.  Coordinates of X and Z lie on the grid 2⁻¹⁰·ℤ inside [0, 4) and s = 1/ℓ is a power of two (1, 2, ½): every scaled
difference e = x·s − z·s is a multiple of 2⁻¹¹ below 8 in magnitude, every e² a multiple of 2⁻²² below 64, and r² = Σ_c e_c² over
d ≤ 128 coordinates a multiple of 2⁻²² below 2¹³ — 35 bits, exact in fp64 whatever the order of summation, with or without fma.  The
device and the host therefore hold the same r² bit for bit (`assert_exact_r2` proves it for a given input set in rationals), and the
products e_c·e_c' of the derivative blocks are exact as well.

Reference values are computed in long double (64-bit significand; mpmath at 40 digits where the platform's long double is no wider than
fp64): `kernel_ref` for the ordinary generator, `grad_blocks` for the four blocks of the gradient-enhanced one and their d/dlog ℓ
forms, each with T, the sum of the magnitudes of the block's terms — the scale of the bound under cancellation.

Plane layout: `plane_offset`, `residues` (oracle.ozaki_oracle.sym_residue on the moduli of the plan, as signed bytes)."""
import math
from fractions import Fraction

import numpy as np

from oracle import gp_oracle as O
from oracle.ozaki_oracle import moduli, sym_residue

LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps < 2e-19)
if not HAVE_LD:                      # a platform whose long double is fp64: 40-digit mpmath behind the same interface
    import mpmath as _mp
    _mp.mp.dps = 40

GRID = 2.0 ** -10
FAMILIES = (O.SE, O.MATERN52, O.MATERN72, O.MATERN32)
GRAD_FAMILIES = (O.SE, O.MATERN52, O.MATERN72)
_SQ = {O.MATERN52: 5, O.MATERN72: 7, O.MATERN32: 3}


# ---- exact inputs -----------------------------------------------------------------------------------------------------------------------
def grid_points(rng, n, d):
    """n points of [0, 4)^d on the grid 2⁻¹⁰·ℤ"""
    return rng.integers(0, 4096, size=(n, d)).astype(np.float64) * GRID


def on_grid(A):
    A = np.asarray(A, dtype=np.float64)
    return bool(np.all(A >= 0) and np.all(A < 4) and np.all(A * 1024 == np.rint(A * 1024)))


def r2_matrix(X, Z, s):
    """r²[j][i] = Σ_c (x_ic·s − z_jc·s)², summed in coordinate order in fp64 (exact: see the module text)"""
    E = X[None, :, :] * s - Z[:, None, :] * s
    r2 = np.zeros(E.shape[:2])
    for c in range(E.shape[2]):
        r2 = r2 + E[:, :, c] * E[:, :, c]
    return r2


def assert_exact_r2(X, Z, s, pairs=64, seed=0):
    """the proof for THIS input set: inputs on the grid, s a power of two, d ≤ 128, and for `pairs` sampled pairs (the extreme rows
    included) the fp64 r² equals the rational one"""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    assert on_grid(X) and on_grid(Z) and X.shape[1] == Z.shape[1] <= 128
    assert s in (0.5, 1.0, 2.0)
    # the general argument, checked on the actual extremes: every e² is a multiple of 2⁻²² and the sum stays below 2³¹·2⁻²²·… < 2⁵³ units
    emax = float(np.max(np.abs(X)) + np.max(np.abs(Z))) * s
    assert X.shape[1] * emax * emax * 2.0 ** 22 < 2.0 ** 53
    r2 = r2_matrix(X, Z, s)
    rng = np.random.default_rng(seed)
    js = np.concatenate([[0, Z.shape[0] - 1], rng.integers(0, Z.shape[0], pairs)])
    is_ = np.concatenate([[0, X.shape[0] - 1], rng.integers(0, X.shape[0], pairs)])
    fs = Fraction(s)
    for j, i in zip(js, is_):
        ex = sum((Fraction(float(X[i, c])) * fs - Fraction(float(Z[j, c])) * fs) ** 2 for c in range(X.shape[1]))
        assert Fraction(float(r2[j, i])) == ex, (j, i)
    return r2


# ---- the input sets of tests/test_gpu_kgen_family.py (tests/test_kgen_ref_cpu.py proves each exact) -------------------------------------
M_STD = 37           # candidates of the ordinary generator's cases: Mc = 48 is two full workgroups and an edge workgroup
DPS = (1, 2, 4, 8, 16, 32)
STD_DIMS = tuple((dp, d) for dp in DPS for d in ((dp, dp - 1) if dp > 1 else (dp,))) + ((64, 40), (96, 70))
GRAD_DIMS = tuple((dp, dp) for dp in DPS) + ((4, 3), (8, 7), (16, 13), (64, 40))
NPS = (128, 640)


def s_of(d):
    """1/ℓ by dimension, so that the kernel values stay well inside the normal range: r² ≤ d·(4s)² ≤ 280 over all cases"""
    return 2.0 if d <= 2 else (1.0 if d <= 8 else 0.5)


def _with_special_candidates(X, Z):
    """two candidates equal to training points, and one that shares every coordinate but the first with a training point (e_c = 0)"""
    Z[0] = X[0]
    Z[-1] = X[-1]
    Z[3] = X[min(7, X.shape[0] - 1)]
    Z[3, 0] = (Z[3, 0] + 0.5) % 4.0
    return Z


def standard_inputs(d, Np, M=M_STD):
    """(X [N = Np − 3][d], Z [M][d], s) of the ordinary generator's case"""
    rng = np.random.default_rng(100000 + 1000 * d + Np)
    X = grid_points(rng, Np - 3, d)
    return X, _with_special_candidates(X, grid_points(rng, M, d)), s_of(d)


def grad_n(d, Np):
    """training points of a gradient case: N·pt ≤ Np − 3 factor rows, the rest of Np is padding"""
    return (Np - 3) // (d + 1)


def grad_inputs(d, Np, M):
    rng = np.random.default_rng(200000 + 1000 * d + Np + 7 * M)
    X = grid_points(rng, grad_n(d, Np), d)
    return X, _with_special_candidates(X, grid_points(rng, M, d)), s_of(d)


def input_sets():
    """every (name, X, Z, s) the GPU tests use"""
    for dp, d in STD_DIMS:
        for Np in NPS:
            yield (f"std dp={dp} d={d} Np={Np}",) + standard_inputs(d, Np)
    for d in (1, 4, 32, 40):
        yield (f"newcol d={d}",) + standard_inputs(d, 128, M=261)
    for dp, d in GRAD_DIMS:
        for Np in NPS:
            for M in (7, 37):
                yield (f"grad dp={dp} d={d} Np={Np} M={M}",) + grad_inputs(d, Np, M)


# ---- long-double kernels ------------------------------------------------------------------------------------------------------------------
def _ld(x):
    return np.asarray(x, dtype=LD)


def _mp_map(fn, u):
    u = np.asarray(u, dtype=np.float64)
    out = np.empty(u.shape, dtype=LD)
    flat, o = u.reshape(-1), out.reshape(-1)
    for n in range(flat.size):
        o[n] = LD(float(fn(_mp.mpf(float(flat[n])))))
    return out


def phis(family, u):
    """φ, φ', φ'', u·φ''' of k = σ_f²·φ(u), u = r² (long double).  Matérn-3/2 has φ only (the others None).
        SE   φ = e^{−u/2}:                  φ' = −φ/2, φ'' = φ/4, uφ''' = −uφ/8
        M52  φ = (1 + ar + 5u/3)E, a = √5:  φ' = −(5/6)(1 + ar)E, φ'' = (25/12)E, uφ''' = −(25/24)·a·r·E
        M72  φ = (1 + ar + 14u/5 + 7a·ur/15)E, a = √7:  φ' = −(7/10)(1 + ar + 7u/3)E, φ'' = (49/60)(1 + ar)E, uφ''' = −(343/120)·u·E
    with r = √u, E = e^{−ar}."""
    if not HAVE_LD:
        return _phis_mp(family, u)
    u = _ld(u)
    if family == O.SE:
        p = np.exp(-u / 2)
        return p, -p / 2, p / 4, -u * p / 8
    a, r = np.sqrt(LD(_SQ[family])), np.sqrt(u)
    E = np.exp(-a * r)
    t = 1 + a * r
    if family == O.MATERN32:
        return t * E, None, None, None
    if family == O.MATERN52:
        return (t + 5 * u / 3) * E, -(LD(5) / 6) * t * E, (LD(25) / 12) * E, -(LD(25) / 24) * a * r * E
    return ((t + LD(14) / 5 * u + 7 * a / 15 * u * r) * E, -(LD(7) / 10) * (t + 7 * u / 3) * E, (LD(49) / 60) * t * E,
            -(LD(343) / 120) * u * E)


def _phis_mp(family, u):
    mp = _mp
    if family == O.SE:
        return (_mp_map(lambda v: mp.exp(-v / 2), u), _mp_map(lambda v: -mp.exp(-v / 2) / 2, u), _mp_map(lambda v: mp.exp(-v / 2) / 4, u),
                _mp_map(lambda v: -v * mp.exp(-v / 2) / 8, u))
    a = mp.sqrt(_SQ[family])
    E = lambda v: mp.exp(-a * mp.sqrt(v))          # noqa: E731
    t = lambda v: 1 + a * mp.sqrt(v)               # noqa: E731
    if family == O.MATERN32:
        return _mp_map(lambda v: t(v) * E(v), u), None, None, None
    if family == O.MATERN52:
        return (_mp_map(lambda v: (t(v) + 5 * v / 3) * E(v), u), _mp_map(lambda v: -mp.mpf(5) / 6 * t(v) * E(v), u),
                _mp_map(lambda v: mp.mpf(25) / 12 * E(v), u), _mp_map(lambda v: -mp.mpf(25) / 24 * a * mp.sqrt(v) * E(v), u))
    return (_mp_map(lambda v: (t(v) + mp.mpf(14) / 5 * v + 7 * a / 15 * v * mp.sqrt(v)) * E(v), u),
            _mp_map(lambda v: -mp.mpf(7) / 10 * (t(v) + 7 * v / 3) * E(v), u), _mp_map(lambda v: mp.mpf(49) / 60 * t(v) * E(v), u),
            _mp_map(lambda v: -mp.mpf(343) / 120 * v * E(v), u))


def kernel_ref(family, r2, sigma_f2):
    """σ_f²·κ(r²) in long double"""
    return LD(sigma_f2) * phis(family, r2)[0]


def kappa_arg(family, r2):
    """the magnitude of the exponential's argument: what the attainable accuracy of κ scales with (test_kappa_device_math)"""
    r2 = np.asarray(r2, dtype=np.float64)
    return 0.5 * r2 if family == O.SE else np.sqrt(_SQ[family] * r2)


def kappa_rel_bound(family, r2):
    """the project's bound of the device's κ against the exact value, relative"""
    return 1.5e-15 + 2.5e-16 * kappa_arg(family, r2)


# ---- the gradient-enhanced generator's blocks -------------------------------------------------------------------------------------------------
def grad_blocks(family, X, Z, s, sigma_f2, dlogell=False, ell_scale=None):
    """V[j][q][i][q'] = cov(output q of candidate z_j, output q' of training point x_i) in long double, with e = (x_i − z_j)·s:
        q = 0,   q' = 0    :  σ_f²·φ
        q = 0,   q' = c'+1 :  σ_f²·s·(2φ'e_c')
        q = c+1, q' = 0    : −σ_f²·s·(2φ'e_c)
        q = c+1, q' = c'+1 : −σ_f²·s²·(4φ''e_c e_c' + 2φ'δ_cc')
    (the header comment of csrc/kgen_grad_core.h); dlogell: the same with φ → −2uφ', φ' → −2uφ'' − 2φ', φ'' → −(2uφ''' + 4φ'').
    Returns (V, T, ND): T the sum of the magnitudes of the terms inside the bracket (without σ_f²·s^q) — for the replaced φ's each of
    their two terms counts separately —, ND[q][q'] the number of derivatives.
    ell_scale (tests of the reference only): evaluate at length scale ℓ·ell_scale, i.e. s/ell_scale, inexact inputs allowed."""
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    sl = LD(s) if ell_scale is None else LD(s) / LD(ell_scale)
    E = _ld(X)[None, :, :] * sl - _ld(Z)[:, None, :] * sl                      # [M][N][d]
    u = np.sum(E * E, axis=2)
    if ell_scale is None:
        u = _ld(r2_matrix(X, Z, s))                                           # the exact fp64 value (identical; keeps mpmath's input fp64)
    p0, p1, p2, up3 = phis(family, u if HAVE_LD else u.astype(np.float64))
    if dlogell:
        f, fT = -2 * u * p1, np.abs(2 * u * p1)
        g, gT = -2 * u * p2 - 2 * p1, np.abs(2 * u * p2) + np.abs(2 * p1)
        h, hT = -(2 * up3 + 4 * p2), np.abs(2 * up3) + np.abs(4 * p2)
    else:
        f, fT, g, gT, h, hT = p0, np.abs(p0), p1, np.abs(p1), p2, np.abs(p2)
    M, N, d = E.shape
    pt = d + 1
    V = np.zeros((M, pt, N, pt), dtype=LD)
    T = np.zeros((M, pt, N, pt), dtype=LD)
    sf = LD(sigma_f2)
    V[:, 0, :, 0], T[:, 0, :, 0] = sf * f, fT
    for c in range(d):
        V[:, 0, :, c + 1] = sf * sl * (2 * g * E[:, :, c])
        V[:, c + 1, :, 0] = -sf * sl * (2 * g * E[:, :, c])
        T[:, 0, :, c + 1] = T[:, c + 1, :, 0] = 2 * gT * np.abs(E[:, :, c])
        for c2 in range(d):
            V[:, c + 1, :, c2 + 1] = -sf * sl * sl * (4 * h * E[:, :, c] * E[:, :, c2] + (2 * g if c == c2 else 0))
            T[:, c + 1, :, c2 + 1] = 4 * hT * np.abs(E[:, :, c] * E[:, :, c2]) + (2 * gT if c == c2 else 0)
    ND = (np.arange(pt)[:, None] > 0).astype(np.int64) + (np.arange(pt)[None, :] > 0).astype(np.int64)
    return V, T, ND


def row_index(M, pc, point_major):
    """(j, q) of the candidate row g = 0 … M·pc − 1 (csrc/kgen_grad_core.h: by outputs, or all outputs of a point adjacent)"""
    g = np.arange(M * pc)
    return (g // pc, g % pc) if point_major else (g % M, g // M)


def as_rows(V, pc, point_major):
    """the 4-index blocks as the generator's matrix: rows g ↔ (j, q < pc) by `point_major`, columns k = i·pt + q' (point-major)"""
    M, _, N, pt = V.shape                 # (the candidate outputs may be cut to q < pc)
    j, q = row_index(M, pc, point_major)
    return V[j, q].reshape(M * pc, N * pt)


# ---- residue planes ---------------------------------------------------------------------------------------------------------------------------
def plane_offset(j, k, res_ld):
    """byte position of (chunk row j, training column k) inside one residue plane: blocks of 256 rows × 64 columns, row-major inside"""
    j, k = np.asarray(j, dtype=np.int64), np.asarray(k, dtype=np.int64)
    return ((j >> 8) * (res_ld >> 6)) * 16384 + (j & 255) * 64 + ((k >> 6) << 14) + (k & 63)


def residues(x, n):
    """[n][…] signed bytes: the symmetric residues of the integer-valued doubles x modulo the n moduli of the plan (p = 256: the low byte)"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((n,) + x.shape, dtype=np.int8)
    for l, p in enumerate(moduli(n)):
        if p == 256:
            out[l] = (x.astype(np.int64) & 255).astype(np.uint8).view(np.int8)
        else:
            out[l] = sym_residue(x, p).astype(np.int8)
    return out


def pad_up(n, m):
    return (n + m - 1) // m * m


def k_scale(kmax):
    """the engine's exponent for values bounded by kmax: |v|·2^sK < 2⁵² (oracle.ozaki_oracle.k_scale)"""
    return 52 - math.frexp(kmax * (1.0 + 1e-12))[1]
