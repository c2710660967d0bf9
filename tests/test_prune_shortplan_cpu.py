"""The short residue plan of the pruned selection's bound pass (csrc/ozaki.hip: "the guarded bound"), restated in
Python integers and fractions.Fraction: the bit split, the row scales, the quantisation and the guard δ_i.  No GPU needed.

What is checked, in exact arithmetic: the short plan's reconstruction Ṽ_ij = (Σ_k W'_ik K'_jk)·2^−(s_i+sK_b) lies within
A(s_i, sK_b) = ½·2^−sK_b·‖W_i‖₁ + ½·2^−s_i·(i+1)·kmax + ¼·(i+1)·2^−(s_i+sK_b) of V_ij = Σ_k W_ik K_jk, and |Σ_k W'_ik K'_jk| < P_b/4
for the bit split the library chooses from the row count.  tests/test_gpu_prune_shortplan.py compares the library's row scales and
guards with the functions of this module."""
import math
from fractions import Fraction

import numpy as np
import pytest

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193]      # csrc/abo_oz_dev.h: oz_mod_p
FULL_MODULI = 14


def plan(n):
    """(P, eP) of the n-modulus plan: 2^eP ≤ P/4 (oz_make_plan)"""
    P = math.prod(MODULI[:n])
    return P, P.bit_length() - 3


def fexp(x):
    """the frexp exponent e(x): x < 2^e"""
    return math.frexp(x)[1]


def bound_kbits(eP, rows):
    """oz_bound_kbits: K' ≤ 2^(bK−1); W keeps eP − bK bits below its row norm — ⌈log₂ rows⌉ more than K"""
    lg = (rows - 1).bit_length()
    return max(2, min(53, (eP - lg) // 2))


def k_scale(kmax, bits=53):
    """oz_k_scale"""
    return bits - 1 - fexp(kmax * (1.0 + 1e-12))


def row_scale(l1, mx, eP, kbits):
    """oz_rowscale_kernel: s_i"""
    return min(eP - kbits - fexp(l1), 52 - fexp(mx))


def pow2(e):
    return Fraction(2) ** e


def guard_A(l1, i, kmax, s, sK):
    """A(s, sK) for row i with L1 norm l1 (exact rationals)"""
    n1 = i + 1
    return Fraction(l1) * pow2(-sK) / 2 + n1 * Fraction(kmax) * pow2(-s) / 2 + Fraction(n1, 4) * pow2(-(s + sK))


def rec_units(n, eP):
    """fp64 reconstruction error of an n-modulus plan, in units of the integer image"""
    return (128 * n * n + 256 * n) * pow2(eP - 91)


def guard_delta(l1, mx, i, sigma_f2, n_b, rows, n_full=FULL_MODULI):
    """(s_i, δ_i) as documented, exact, on the exact row norm l1 — without the inflations the kernel applies on top:
    l1 → l1·(1 + (i+1)·2^-52) and the closing factor 1 + 2^-40"""
    _, eP_b = plan(n_b)
    _, eP_f = plan(n_full)
    bK = bound_kbits(eP_b, rows)
    sK_b, sK_f = k_scale(sigma_f2, bK), k_scale(sigma_f2)
    kmax = Fraction(sigma_f2) * (1 + pow2(-40))
    s = row_scale(l1, mx, eP_b, bK)
    sf = row_scale(l1, mx, eP_f, 53)
    Ab, Af = guard_A(l1, i, kmax, s, sK_b), guard_A(l1, i, kmax, sf, sK_f)
    d = Ab + Af + rec_units(n_b, eP_b) * pow2(-(s + sK_b)) + rec_units(n_full, eP_f) * pow2(-(sf + sK_f)) + \
        pow2(-50) * (Fraction(l1) * kmax + Ab + Af)
    return s, d


def quantise(x, s):
    """rint(x·2^s) as Python integers (the scaling by a power of two is exact, rint rounds half to even as the device does)"""
    return [int(v) for v in np.rint(np.ldexp(np.asarray(x, dtype=np.float64), s))]


def _rows(rng, R, sigma_f2):
    """(row index, row) cases: random rows with norms over 2^-20 … 2^20, all-equal rows, one dominant entry, at the row indices
    where the (i+1) term matters: the first, around a 128-row boundary, the last of a 256-row block"""
    out = []
    for i in (0, 1, 63, 127, 128, 254, 255):
        if i >= R:
            continue
        out.append((i, rng.standard_normal(i + 1) * 2.0 ** rng.uniform(-20, 20)))
        out.append((i, np.full(i + 1, 2.0 ** rng.integers(-20, 20) * 0.7)))                   # all equal: worst case of the (i+1) term
        w = rng.standard_normal(i + 1) * 1e-6
        w[i] = 3.0 * 2.0 ** rng.integers(-20, 20)                                             # L1 ≈ max: the 52 − e(mx) branch where bW > 52
        out.append((i, w))
    return out


@pytest.mark.parametrize("n_b,expect_mx_branch", [(8, False), (9, False), (10, False), (13, True)])
def test_reconstruction_within_the_guard(n_b, expect_mx_branch):
    rng = np.random.default_rng(1234 + n_b)
    R, sigma_f2 = 256, 1.7
    P, eP = plan(n_b)
    bK = bound_kbits(eP, R)
    sK = k_scale(sigma_f2, bK)
    kmax = Fraction(sigma_f2) * (1 + pow2(-40))
    took_mx_branch = False
    for i, w in _rows(rng, R, sigma_f2):
        l1 = sum(Fraction(abs(float(v))) for v in w)
        mx = float(np.max(np.abs(w)))
        s = row_scale(float(l1), mx, eP, bK)
        took_mx_branch = took_mx_branch or s == 52 - fexp(mx) < eP - bK - fexp(float(l1))
        Wq = quantise(w, s)
        A = guard_A(l1, i, kmax, s, sK)
        _, delta = guard_delta(l1, mx, i, sigma_f2, n_b, R)
        assert delta >= A
        for K in (rng.uniform(0.0, sigma_f2, i + 1), np.full(i + 1, sigma_f2), np.zeros(i + 1),
                  np.full(i + 1, sigma_f2 * (1.0 + 2.0 ** -41))):
            Kq = quantise(K, sK)
            assert max(Kq) <= 2 ** (bK - 1)
            acc = sum(a * b for a, b in zip(Wq, Kq))
            assert 4 * abs(acc) < P
            Vt = Fraction(acc) * pow2(-(s + sK))
            V = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(w, K))
            assert abs(Vt - V) <= A, (n_b, i, float(abs(Vt - V)), float(A))
    assert took_mx_branch == expect_mx_branch


def test_full_plan_term_of_the_guard_on_the_max_branch():
    """For the plans the library accepts (8 – 10 moduli) the `52 − e(max)` branch never sets the SHORT plan's scale (the case n_b = 13
    above is the restatement's only); it does set the FULL plan's scale of a row whose norm is within a factor 4 of its largest entry,
    and that scale enters δ through A(s'', sK'').  Such rows, in exact arithmetic: the 14-modulus image lies within that term."""
    rng = np.random.default_rng(77)
    sigma_f2 = 1.7
    _, eP_f = plan(FULL_MODULI)
    sK_f = k_scale(sigma_f2)
    kmax = Fraction(sigma_f2) * (1 + pow2(-40))
    for i in (0, 5, 127, 255):
        w = rng.standard_normal(i + 1) * 1e-9
        w[i // 2] = -1.37 * 2.0 ** int(rng.integers(-20, 20))
        l1 = sum(Fraction(abs(float(v))) for v in w)
        mx = float(np.max(np.abs(w)))
        sf = row_scale(float(l1), mx, eP_f, 53)
        assert sf == 52 - fexp(mx) < eP_f - 53 - fexp(float(l1))
        s, delta = guard_delta(l1, mx, i, sigma_f2, 8, 256)
        assert s == plan(8)[1] - bound_kbits(plan(8)[1], 256) - fexp(float(l1))              # the short plan: the norm branch
        Af = guard_A(l1, i, kmax, sf, sK_f)
        assert delta >= Af + guard_A(l1, i, kmax, s, k_scale(sigma_f2, bound_kbits(plan(8)[1], 256)))
        Kv = rng.uniform(0.0, sigma_f2, i + 1)
        acc = sum(a * b for a, b in zip(quantise(w, sf), quantise(Kv, sK_f)))
        V = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(w, Kv))
        assert abs(Fraction(acc) * pow2(-(sf + sK_f)) - V) <= Af


@pytest.mark.parametrize("n_b", [8, 9, 10])
@pytest.mark.parametrize("R", [256, 1024, 4096])
def test_integer_sums_stay_below_a_quarter_of_P(n_b, R):
    P, eP = plan(n_b)
    assert 2 ** eP <= P // 4
    bK = bound_kbits(eP, R)
    assert 2 <= bK <= 53 and eP - bK - bK in ((R - 1).bit_length(), (R - 1).bit_length() + 1)     # W gets ⌈log₂R⌉ (+1) more bits
    # the analytic bound: 2^s·L1 < 2^(eP−bK) (L1 < 2^e(L1)), |W'| ≤ |W|·2^s + ½, K' ≤ 2^(bK−1)
    assert (pow2(eP - bK) + Fraction(R, 2)) * 2 ** (bK - 1) < Fraction(P, 4)
    # and an adversarial last row: L1 just below a power of two, every K at a σ_f² just below a power of two
    i = R - 1
    sigma_f2 = 2.0 - 2.0 ** -40
    w = np.full(i + 1, (1.0 - 2.0 ** -30) / (i + 1))
    w[::2] *= -1.0
    l1 = float(sum(Fraction(abs(float(v))) for v in w))
    s = row_scale(l1, float(np.max(np.abs(w))), eP, bK)
    Wq = [abs(v) for v in quantise(w, s)]
    Kq = quantise(np.full(i + 1, sigma_f2 * (1.0 + 2.0 ** -41)), k_scale(sigma_f2, bK))
    assert 4 * sum(a * b for a, b in zip(Wq, Kq)) < P


def test_the_default_plan_at_the_flagship_shape():
    _, eP = plan(8)
    assert eP == 61 and bound_kbits(eP, 1024) == 25 and eP - 25 == 36          # K 25 bits, W 36 bits below its row norm
    assert k_scale(1.0) == 51 and k_scale(1.0, 25) == 23                       # σ_f² = 1 < 2^1
