"""Reference of the factorisation family (csrc/chol.hip and the blocked driver of csrc/api.hip) — NumPy, no GPU.  TEST INFRASTRUCTURE ONLY.

Exact family.  L₀ = (I + E)·D with D = diag(2^e), e ∈ {0, 1, 2}, and E integer in [−3, 3], non-zero only at (odd row, even column,
column < row).  A row of E reaches even columns only and a column of E is fed by odd rows only, so E² = 0 and L₀⁻¹ = D⁻¹(I − E) exactly:
the factor holds small integers, its inverse multiples of ¼, A = L₀L₀ᵀ small integers of both signs.  Every pivot A_jj − Σ_k L_jk² =
L_jj² is a power of four, every pair determinant a·d0 − b² = (L_jj·L_{j+1,j+1})² as well, and every Schur complement, every partial
sum of the factorisation and of the inversion is a dyadic number far below 2⁵³ units of its grid (`assert_exact` proves it for a given
size with integers): whatever order a kernel sums in, and with or without fma, the expected L, W = L⁻¹ and WT = Wᵀ are known bit for bit.

Signed SPD family: A = GGᵀ/n + I with Gaussian G — entries of both signs, κ₂ ≲ 10.

Conditioning ladder: SE and Matérn-5/2 kernel matrices (σ_f² = 1) of clustered points — synth.points squeezed into a tenth of the
box — plus noise ∈ {1e-4, 1e-6, 1e-8, 1e-10} on the diagonal: the small-noise GP regime.

Measures (all evaluated at least 2¹⁰ below what they measure: in long double up to n = 640, above that — and wherever long double is
no wider than fp64 — by sliced exact products, `resid`):
    eta(A, L)     = max|A − LLᵀ| / max|A|                           normwise backward error
    rho(A, L)     = max_ij |A − LLᵀ|_ij / (|L||L|ᵀ)_ij              componentwise (Higham, ASNA 2nd ed., Thm 10.3: ≤ γ_{n+1} for LAPACK's)
    inv_res(L, W) = max_ij |WL − I|_ij / (|W||L|)_ij                left residual of the triangular inverse
    kappa16(L)    = max κ₂ over the 16×16 diagonal sub-blocks of L  the factor a solve through explicit 16×16 inverses carries"""
from fractions import Fraction

import numpy as np

from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O

LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps < 2e-19)
U = 2.0 ** -53
LD_MAX_N = 640
NOISES = (1e-4, 1e-6, 1e-8, 1e-10)
LADDER_FAMILIES = (O.SE, O.MATERN52)
SENTINEL = 2.0 ** 40


# ---- exact family -----------------------------------------------------------------------------------------------------------------------
def exact_factor(n, seed=0):
    """(L₀, L₀⁻¹) of the module text, n × n, both exact in fp64"""
    rng = np.random.default_rng(1000 + seed)
    E = np.zeros((n, n))
    odd, even = np.arange(1, n, 2), np.arange(0, n, 2)
    if len(odd):
        blk = rng.integers(-3, 4, size=(len(odd), len(even))).astype(np.float64)
        blk[even[None, :] >= odd[:, None]] = 0.0
        E[np.ix_(odd, even)] = blk
    dg = 2.0 ** rng.integers(0, 3, size=n)
    I = np.eye(n)
    return (I + E) * dg[None, :], (I - E) / dg[:, None]


def exact_case(n, seed=0):
    """(A, L₀, L₀⁻¹): A = L₀L₀ᵀ, an exact integer matrix (the fp64 product is exact: assert_exact)"""
    L0, W0 = exact_factor(n, seed)
    return L0 @ L0.T, L0, W0


def assert_exact(L0, W0):
    """the proof for THIS factor: on the grid of ¼ every entry of L₀ and W₀ is an integer, and the sums of MAGNITUDES
    Σ_k |L_ik||L_jk| (the factorisation: every Schur complement and partial sum of A − Σ L·L lies below |A| plus it) and
    Σ |W||L||W| (the inversion, W21 = −W22·L21·W11, with its intermediate |L||W|) stay below 2⁵³ grid units — so no partial sum, in
    any order, with or without fma, ever rounds.  The magnitude sums are sums of NON-NEGATIVE integers: a floating-point sum of those is
    monotone, so a computed value below 2⁵³ means no partial sum reached 2⁵³ and the computed value is the true one.  The identities
    L₀·L₀⁻¹ = I and A = L₀L₀ᵀ are checked in rationals on sampled rows (the extremes included)."""
    n = L0.shape[0]
    Li, Wi = np.abs(L0 * 4.0), np.abs(W0 * 4.0)
    assert np.all(Li == np.rint(Li)) and np.all(Wi == np.rint(Wi))
    s_fact = 2 * int((Li @ Li.T).max())                        # |A| + Σ|L||L| ≤ 2·Σ|L||L|, in units of ¹⁄₁₆
    LW = Li @ Wi
    s_mid = int(LW.max())                                      # |L21||W11| in units of ¹⁄₁₆
    s_inv = int((Wi @ LW).max())                               # |W22||L21||W11| in units of ¹⁄₆₄
    assert max(s_fact, s_mid, s_inv) < 2 ** 53, (s_fact, s_mid, s_inv)
    A = L0 @ L0.T
    for i in sorted({0, 1, n - 1, n // 2}):
        Lr = [Fraction(float(v)) for v in L0[i]]
        for j in sorted({0, 1, max(i - 1, 0), i, n // 3, n - 1}):
            assert sum(Lr[k] * Fraction(float(W0[k, j])) for k in range(i + 1)) == Fraction(int(i == j)), (i, j)
            assert Fraction(float(A[i, j])) == sum(Lr[k] * Fraction(float(L0[j, k])) for k in range(n)), (i, j)
    return max(s_fact, s_mid, s_inv)


# ---- signed SPD family and the conditioning ladder ----------------------------------------------------------------------------------------
def signed_spd(n, seed=0):
    G = np.random.default_rng(2000 + seed).standard_normal((n, n))
    A = G @ G.T / n
    A = 0.5 * (A + A.T)
    A[np.diag_indices(n)] += 1.0
    return A


def ladder_points(n, d=3, seed=11):
    """synth.points squeezed into a tenth of the unit box"""
    return 0.45 + 0.1 * synth.points(seed, n, d)


def ladder_matrix(family, noise, n):
    X = ladder_points(n)
    A = O.kernel_matrix(family, 1.0, 1.0, X)
    A = 0.5 * (A + A.T)
    A[np.diag_indices(n)] += noise
    return A


def ladder_cases(n):
    """[(name, A, κ₂(A))] over families × noises; the name carries κ₂"""
    out = []
    for fam in LADDER_FAMILIES:
        for nz in NOISES:
            A = ladder_matrix(fam, nz, n)
            kap = float(np.linalg.cond(A))
            out.append((f"{'se' if fam == O.SE else 'm52'}_noise{nz:.0e}_kappa{kap:.1e}", A, kap))
    return out


# ---- measures ---------------------------------------------------------------------------------------------------------------------------
def _slices(X):
    """rows of X as four 16-bit integer slices against the row maximum: X[i] = Σ_s S[s][i]·2^(e[i] − 16·(s+1)) up to 2^(e[i] − 64)"""
    X = np.asarray(X, dtype=np.float64)
    m = np.max(np.abs(X), axis=1)
    e = np.where(m > 0, np.frexp(np.where(m > 0, m, 1.0))[1], 0)           # |X[i]| < 2^e[i]
    R = np.ldexp(X, -e[:, None])                                           # |R| < 1, exact
    S = []
    for _ in range(4):
        R = R * 65536.0
        T = np.trunc(R)
        S.append(T)
        R = R - T                                                          # exact: |R| < 1 again
    return S, e


def resid_sliced(Cm, X, Y):
    """C − X·Yᵀ with every slice product exact in fp64 BLAS (|slice| < 2¹⁶, n ≤ 2048: sums below 2⁴³); the sixteen products are summed
    from the smallest scale to the largest, the largest is subtracted from C first"""
    assert X.shape[1] == Y.shape[1] <= 2048
    Sx, ex = _slices(X)
    Sy, ey = _slices(Y)
    sc = (ex[:, None] + ey[None, :]).astype(np.int64)
    tail = np.zeros(Cm.shape)
    for lvl in range(6, 0, -1):                                            # s + t = lvl: scale 2^(−16·(lvl + 2))
        P = sum(Sx[s] @ Sy[lvl - s].T for s in range(4) if 0 <= lvl - s < 4)
        tail = tail + np.ldexp(P, sc - 16 * (lvl + 2))
    head = np.ldexp(Sx[0] @ Sy[0].T, sc - 32)
    return (np.asarray(Cm, dtype=np.float64) - head) - tail


def resid(Cm, X, Y):
    """C − X·Yᵀ: long double up to n = 640, sliced exact products above (and where long double is fp64)"""
    if HAVE_LD and X.shape[1] <= LD_MAX_N and max(X.shape[0], Y.shape[0]) <= LD_MAX_N:
        return np.asarray(Cm.astype(LD) - X.astype(LD) @ Y.astype(LD).T, dtype=np.float64)
    return resid_sliced(Cm, X, Y)


def backward(A, L):
    """(eta, rho) of the module text from ONE evaluation of A − LLᵀ"""
    r = np.abs(resid(A, L, L))
    den = np.abs(L) @ np.abs(L).T
    return float(np.max(r) / np.max(np.abs(A))), float(np.max(r[den > 0] / den[den > 0]))


def eta(A, L):
    return backward(A, L)[0]


def rho(A, L):
    return backward(A, L)[1]


def inv_res(L, W):
    n = L.shape[0]
    den = np.abs(W) @ np.abs(L)
    r = np.abs(resid(np.eye(n), W, np.ascontiguousarray(L.T)))
    return float(np.max(r[den > 0] / den[den > 0]))


def kappa16(L):
    n = L.shape[0]
    assert n % 16 == 0
    return float(max(np.linalg.cond(L[o:o + 16, o:o + 16]) for o in range(0, n, 16)))


def panel_res(Ap, X, Lbb):
    """normwise relative residual of X·L_bbᵀ = A_panel: max|A_p − X·L_bbᵀ| / max(|X|·|L_bb|ᵀ)"""
    return float(np.max(np.abs(resid(Ap, X, Lbb))) / np.max(np.abs(X) @ np.abs(Lbb).T))


def gamma(k):
    return k * U / (1.0 - k * U)


def inv_bar(kap16):
    """the known bound of a solve through explicit 16×16 inverses"""
    return 16.0 * U * kap16


def ulp_diff(a, b):
    """|a − b| in units in the last place of b (finite fp64 arrays)"""
    return np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.abs(np.asarray(b)))
