"""Plain numpy references of the selection family (csrc/misc.hip), independent of the device's order-preserving u64 keys: what
tests/test_gpu_select_family.py holds the kernels against, and what tests/test_select_ref_cpu.py checks on its own.

  sortperm_rev     Julia's sortperm(scores; rev=true)[1:k] from isless: NaN (either sign, any payload) first, then the values descending
                   with 0.0 ahead of −0.0, ties by ascending index
  topk_expect      the (index, value bits) pairs launch_topk must write for k requested entries
  prune_keep_ref   the guard !(ub + |ub|·2⁻³⁰ + abs < tau) in fp64
  finalize_ref     the epilogue's additions in the kernel's order, elementwise in fp64 (every comparison is an equality)
  fma_ref          fma(c, β, μ) in long double, rounded once
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = 2.0 ** 40                       # finite: a kernel that reads behind the logical width of an input shows in the result
QNAN_BITS = np.uint64(0x7ff8000000000000)  # what the selection writes behind the last real entry
PRUNE_REL = 2.0 ** -30
FAMILIES = "abcdefg"


def gamma(k):
    return k * U / (1.0 - k * U)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def sortperm_rev(scores, k):
    """0-based indices of the first min(k, len) entries in Julia's isless-descending, stable order"""
    s = np.asarray(scores, dtype=np.float64)
    n = s.shape[0]
    nan = np.isnan(s)
    val = np.where(nan, 0.0, s)
    zero_sign = ((val == 0.0) & np.signbit(val)).astype(np.int8)          # among the zeros: 0.0 (rank 0) ahead of −0.0 (rank 1)
    order = np.lexsort((np.arange(n), zero_sign, -val, (~nan).astype(np.int8)))   # the LAST key is the primary one
    return order[:max(0, min(int(k), n))].astype(np.int64)


def topk_expect(scores, M, k, idx_base):
    """top_idx [k] and the bit patterns of top_val [k]: the selected entries' own bits (a NaN's payload comes back as it went in),
    then (canonical quiet NaN, −1) behind the min(k, M) real ones"""
    s = np.asarray(scores, dtype=np.float64)[:M]
    sel = sortperm_rev(s, k)
    idx = np.full(k, -1, dtype=np.int64)
    val = np.full(k, QNAN_BITS, dtype=np.uint64)
    idx[:sel.size] = sel + idx_base
    val[:sel.size] = bits(s)[sel]
    return idx, val


def nan_with(sign, payload):
    """a NaN with that sign bit and mantissa (1 ≤ payload < 2⁵²; the quiet bit is whatever the payload says)"""
    assert 1 <= payload < 2 ** 52
    return from_bits(np.array([(sign << 63) | (0x7ff << 52) | payload], dtype=np.uint64))[0]


SPECIALS = [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1030, -(2.0 ** -1030), np.finfo(np.float64).max, -np.finfo(np.float64).max,
            nan_with(0, 1 << 51), nan_with(1, 1 << 51), nan_with(0, 0x123456789), nan_with(1, 1), 0.0, -0.0, np.inf, -np.inf]


def special_places(M):
    """where family (e) puts SPECIALS[i]: spread over the batch, both ends included; on a batch shorter than the list the later
    ones overwrite the earlier"""
    n = len(SPECIALS)
    return [0 if M == 1 else (i * (M - 1)) // (n - 1) for i in range(n)]


def scores_family(fam, M, seed):
    """the score families of the top-k tests, drawn on the host from a seeded generator"""
    rng = np.random.default_rng([seed, M, ord(fam)])
    if fam == "a":                                      # tie-free normals
        s = rng.standard_normal(M)
        assert np.unique(s).size == M
    elif fam == "b":                                    # three distinct values: the k-th entry sits inside a run of ties
        s = rng.choice(np.array([-1.5, 0.25, 2.0]), size=M)
    elif fam == "c":                                    # all equal
        s = np.full(M, 0.75)
    elif fam == "d":                                    # all NaN, mixed signs and payloads
        b = (rng.integers(0, 2, size=M, dtype=np.uint64) << np.uint64(63)) | np.uint64(0x7ff << 52) | \
            rng.integers(1, 2 ** 52, size=M, dtype=np.uint64)
        s = from_bits(b)
        assert np.isnan(s).all()
    elif fam == "e":                                    # ±Inf, ±0.0, subnormals, ±DBL_MAX and NaNs at known places among normals
        s = rng.standard_normal(M)
        for place, v in zip(special_places(M), SPECIALS):
            s[place:place + 1] = v
    elif fam == "f":                                    # keys that agree in their top seven bytes: all eight radix passes
        s = 1.0 + (np.arange(M) % 256) * 2.0 ** -52
    elif fam == "g":                                    # all negative
        s = -np.abs(rng.standard_normal(M)) - 2.0 ** -20
    else:
        raise ValueError(fam)
    return np.ascontiguousarray(s, dtype=np.float64)


def prune_keep_ref(ub, tau, abs_margin):
    """keep[j] = !(ub[j] + |ub[j]|·2⁻³⁰ + abs_margin < tau): a NaN on either side, and −Inf + Inf, keep the candidate"""
    ub = np.asarray(ub, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        guard = ub + np.abs(ub) * PRUNE_REL + np.float64(abs_margin)
        return ~(guard < np.float64(tau))


def guard_boundary(tau, abs_margin, steps=(-2, -1, 0, 1, 2)):
    """bounds whose guard lies within an ulp or two either side of a finite, normal tau: the ub nearest tau/(1 + 2⁻³⁰) and its neighbours"""
    x = np.float64((LD(tau) - LD(abs_margin)) / (LD(1) + LD(math.copysign(PRUNE_REL, tau))))
    out = []
    for st in steps:
        y = x
        for _ in range(abs(st)):
            y = np.nextafter(y, np.inf if st > 0 else -np.inf)
        out.append(y)
    return np.array(out, dtype=np.float64)


def finalize_ref(partial, mu_in, M, j0, Mc, T, sigma_f2, prior_grad=0.0, pc=1, point_major=0, Mpts=0, mu_tail=None, mu_eps=None,
                 head_g=None, ssq_g=None, n_out=None, fill=np.nan):
    """(mu_out, var_out, mu_tail_out) over the GLOBAL index range [0, n_out) (default: the length of mu_tail / head_g, else M): rows
    j0 ≤ gj < min(j0 + Mc, M) as finalize_kernel computes them, everything else `fill` (mu_tail_out: the input elsewhere).  Additions
    in the kernel's order, one fp64 rounding each."""
    n_glob = n_out if n_out is not None else len(mu_tail) if mu_tail is not None else len(head_g) if head_g is not None else M
    mu_out, var_out = np.full(n_glob, fill), np.full(n_glob, fill)
    tail_out = None if mu_tail is None else np.array(mu_tail, dtype=np.float64)
    hi = min(j0 + Mc, M)
    if hi <= j0:
        return mu_out, var_out, tail_out
    gj = np.arange(j0, hi)
    j = gj - j0
    q = np.zeros(gj.size) if ssq_g is None else np.array(ssq_g, dtype=np.float64)[gj]
    for t in range(T):
        q = q + partial[t, j]                                      # row blocks in order
    prior = np.full(gj.size, np.float64(sigma_f2))
    if pc > 1:
        o = gj % pc if point_major else gj // Mpts
        prior[o > 0] = prior_grad
    var = (prior - q) + 1e-18
    mu = np.array(head_g, dtype=np.float64)[gj] if head_g is not None else np.array(mu_in, dtype=np.float64)[j]
    if mu_tail is not None:
        mu = mu + np.asarray(mu_tail, dtype=np.float64)[gj]
        tail_out[gj] = mu
        mu = mu - np.asarray(mu_eps, dtype=np.float64)[gj]
    mu_out[gj], var_out[gj] = mu, var
    return mu_out, var_out, tail_out


def guarded(sc, abs_margin):
    """the bound pass's stored score: sc + |sc|·2⁻³⁰ + abs for a finite sc, an infinite one as it is"""
    sc = np.asarray(sc, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        g = sc + np.abs(sc) * PRUNE_REL + np.float64(abs_margin)
    return np.where(np.isinf(sc), sc, g)


def fma_ref(c, beta, mu):
    """fma(c, β, μ): product and sum in long double (64-bit significand), ONE rounding to fp64.  Exact only where the long double
    holds product and sum exactly — downdate_operands() draws such operands, tests/test_select_ref_cpu.py proves it with rationals."""
    return (np.asarray(c, dtype=LD) * LD(beta) + np.asarray(mu, dtype=LD)).astype(np.float64)


def downdate_operands(M, seed):
    """c, β ∈ ±[1, 2) on the grid 2⁻²⁹ (30 bits each: the product has up to 60, more than fp64 holds — a multiply followed by an add
    rounds twice and differs from the fma — and is exact in long double), μ ∈ ±[1, 4) on the grid 2⁻⁵⁰: product + μ is a multiple of
    2⁻⁵⁸ below 8, 61 bits, exact in long double as well.  var, s2: anything positive."""
    rng = np.random.default_rng([seed, M])
    grid = lambda n: (1.0 + rng.integers(0, 2 ** 29, size=n) * 2.0 ** -29) * rng.choice([-1.0, 1.0], size=n)
    c = grid(M)
    beta = float(grid(1)[0])
    mu = (1.0 + rng.integers(0, 3 * 2 ** 50, size=M) * 2.0 ** -50) * rng.choice([-1.0, 1.0], size=M)
    var = rng.uniform(0.5, 2.0, size=M)
    s2 = float(rng.uniform(0.5, 2.0))
    return c, beta, mu, var, s2


def gradnorm_ref(m, C, beta):
    """GradientNormUCB of one point in long double on the gradient block (outputs 1 … p − 1) of the mean m [p] and covariance C [p][p],
    and the a-priori bound on the fp64 evaluation of gradnorm_moments / gradnorm_ucb (csrc/abo_acq_dev.h), n = p − 1, u = 2⁻⁵³:
      mm = Σ m_q²            n fmas in turn                       |δ| ≤ γ_n·mm
      tr = Σ C_qq            n additions                          |δ| ≤ γ_n·Σ|C_qq|
      msm = Σ_q m_q·row_q    row_q: n fmas, then one fma per q    |δ| ≤ γ_2n·A,  A = Σ_q Σ_q' |m_q||C_qq'||m_q'|
      fro = Σ C_qq'²         n² fmas in turn                      |δ| ≤ γ_n²·fro
      ms = mm + tr           one more rounding                    |δ| ≤ γ_(n+1)·(mm + Σ|C_qq|)
      vs = 4·msm + 2·fro     exact scalings, one rounding         |δ| ≤ 4γ_(2n+1)·A + 2γ_(n²+1)·fro =: e_vs
      s = sqrt(max(vs, 1e-12))   |√a − √b| ≤ |a − b|/√b, the root itself within 2u      |δ| ≤ e_vs/√v + 2u·s
      score = −ms + β·s      the product and the sum (or one fma) |δ| ≤ δms + |β|·δs + 2u·(|ms| + |β|·s)
    Returns (score, bar)."""
    p = m.shape[0]
    n = p - 1
    g, S = m[1:].astype(LD), C[1:, 1:].astype(LD)
    mm, diag = np.sum(g * g), np.sum(np.abs(np.diag(S)))
    tr = np.sum(np.diag(S))
    msm, A = g @ S @ g, np.abs(g) @ np.abs(S) @ np.abs(g)
    fro = np.sum(S * S)
    ms = mm + tr
    v = max(LD(4) * msm + LD(2) * fro, LD(1e-12))
    s = np.sqrt(v)
    score = -ms + LD(beta) * s
    if n == 0:
        return float(score), 4 * U * float(abs(beta) * s)
    e_ms = gamma(n + 1) * float(mm + diag)
    e_vs = 4 * gamma(2 * n + 1) * float(A) + 2 * gamma(n * n + 1) * float(fro)
    e_s = e_vs / float(s) + 2 * U * float(s)
    bar = (e_ms + abs(beta) * e_s + 2 * U * (float(abs(ms)) + abs(beta) * float(s))) * (1 + 2.0 ** -20)
    return float(score), bar
