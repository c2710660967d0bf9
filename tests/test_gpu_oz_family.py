"""Direct tests of the int8 residue engine (csrc/ozaki.hip), stage by stage (-m gpu), through the abo_test_oz_* hooks of the test build:
(a) row scales and the guard, (b) the quantiser, (c) the GEMM epilogue's residue arithmetic, (d) the persistent residue GEMM, (e) the
reconstruction to V, (f) the reconstruction to column sums in every instantiation, (g) the stages chained against the one-call contraction.

Method (tests/oz_ref.py; its own checks: tests/test_oz_ref_cpu.py).  Integer stages — scales, residue bytes, U — are equalities against
Python integers; the reconstructions are held to the project's own bound rec = (128n² + 256n)·2^(eP−91) integer units (ozaki.hip: "the
guarded bound") in exact rational arithmetic, reached / bound recorded through check().  Every output starts as a sentinel (NaN for
doubles, 0x5A for bytes and ints) and is checked where the stage must not write."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import ABO_EINVAL, AboTestOzQuantArgs

from tests import oz_ref as R
from tests.parity_record import check

NAN, INF = float("nan"), float("inf")
SENT = 0x5A
SENT32 = 0x5A5A5A5A
eq = np.testing.assert_array_equal


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return t.data_ptr() if t is not None else None


def lib():
    return abo._lib.lib()


def ok(status):
    abo._lib.check(status)


def sent_bytes(n):
    return dev(np.full(n, SENT, dtype=np.uint8).view(np.int8))


def sent_ints(n):
    return dev(np.full(n, SENT32, dtype=np.int32))


# ---- (a) row scales ---------------------------------------------------------------------------------------------------------------------
LADDER = list(range(-1040, 991, 70)) + [-1022, -975, -960, -905, 990]


def rowscale_matrix():
    """384 rows (370 valid) of a lower-triangular W.  Every row's entries are small integers (≤ 2^20) times ONE power of two, or two
    terms: every partial sum of a row is then exact in fp64 whatever the order, so the wave's L1 equals math.fsum's and cannot sit on the
    other side of a power of two."""
    rng = np.random.default_rng(5)
    W = np.zeros((384, 384))
    kinds = {}
    for i in range(384):
        W[i, :i + 1] = rng.integers(-2 ** 20, 2 ** 20, i + 1) * 2.0 ** int(rng.integers(-60, 60))       # L1 ≫ max from a few entries on
    W[7, :8] = [1, -1, 1, 1, -1, 1, 1, 1]; kinds[7] = "tie"                     # L1 = 8, max = 1: eP − 53 − 4 = 52 − 1 at 14 moduli
    W[9, :10] = 0; W[9, 3] = -3.0; W[9, 0] = 2.0 ** -30; kinds[9] = "max"       # one dominant entry: the max branch
    # L1 one ulp below 1 and exactly 1, from 32 entries of 2^-5 (one of them 2^-53 short): every partial sum is a multiple of 2^-53 below
    # 1, exact in any order; max = 2^-5 leaves the L1 branch to decide (eP − 53 − e(L1) = 55 against 54 at 14 moduli; 52 − e(max) = 56)
    W[50, :51] = 0; W[50, :32] = -(2.0 ** -5); W[50, 17] = 2.0 ** -5 - 2.0 ** -53; kinds[50] = "below"
    W[51, :52] = 0; W[51, :32] = 2.0 ** -5; kinds[51] = "at"
    W[20, :21] = 0; kinds[20] = "zero"
    W[21, 4] = NAN; kinds[21] = "nan"
    W[22, 0] = -INF; kinds[22] = "inf"
    W[23, :24] = 0; W[23, [0, 4, 8, 12]] = [5e299, -5e299, 5e299, 5e299]; kinds[23] = "overflow"   # every entry < 1e300, L1 = 2e300
    for q, e in enumerate(LADDER):                                               # norms 2^-1040 (subnormal entries) … 2^990
        i = 100 + 3 * q
        W[i, :i + 1] = 0
        W[i, :5] = np.ldexp([1.0, -3.0, 2.0, 1.0, 1.0], e - 3)
        kinds[i] = ("ladder", e)
    return W, kinds


def ref_scales(W, nrows, n, kbits, kper, ktg):
    eP = R.plan(n)["eP"]
    out = np.zeros(W.shape[0] if W.shape[0] % 256 == 0 else (W.shape[0] // 256 + 1) * 256, dtype=np.int64)
    norms = []
    for i in range(nrows):
        w = np.abs(W[i, :i + 1]) * np.where((kper > 1) & (np.arange(i + 1) % kper != 0), 2.0 ** ktg, 1.0)
        l1, mx = math.fsum(w), (float(np.nanmax(w)) if not np.all(np.isnan(w)) else 0.0)
        out[i] = R.row_scale(l1, mx, eP, kbits, ktg if kper > 1 else 0)
        norms.append((l1, mx))
    return out, norms


@pytest.mark.parametrize("n,kbits,kper,ktg", [(14, 53, 1, 0), (14, 53, 4, 7), (14, 53, 4, -7), (16, 53, 1, 0), (8, 25, 1, 0)])
def test_row_scales_equal_the_rule(n, kbits, kper, ktg):
    W, kinds = rowscale_matrix()
    nrows, rows256 = 370, 512
    sexp, Wd = sent_ints(rows256 + 8), dev(W)
    ok(lib().abo_test_oz_rowscale(0, ptr(Wd), 384, nrows, rows256, n, kper, ktg, kbits, 0, 0, 0, 0.0, 0.0, 0.0, ptr(sexp), None))
    got = host(sexp)
    want, _ = ref_scales(W, nrows, n, kbits, kper, ktg)
    eq(got[:rows256], want)                                  # rows ≥ nrows: 0
    eq(got[rows256:], np.full(8, SENT32))
    for i in (21, 22, 23):
        assert want[i] == R.SEXP_BAD
    clamp = R.SEXP_MAX - max(ktg if kper > 1 else 0, 0)
    assert want[20] == 0 and want.max() == clamp and (want == clamp).sum() >= 2        # the bottom of the ladder sits on the clamp


def test_guard_delta_against_its_restatement():
    W, kinds = rowscale_matrix()
    nrows, rows256, sf2, n_b, n_f = 370, 512, 1.7, 8, 14
    eP_b, eP_f = R.plan(n_b)["eP"], R.plan(n_f)["eP"]
    bK = R.bound_kbits(eP_b, rows256)
    sK_b, sK_f = R.k_scale(sf2, bK), R.k_scale(sf2)
    sexp, delta, Wd = sent_ints(rows256), dev(np.full(rows256 + 4, NAN)), dev(W)
    ok(lib().abo_test_oz_rowscale(0, ptr(Wd), 384, nrows, rows256, n_b, 1, 0, bK, eP_f, sK_b, sK_f, sf2 * (1.0 + 2.0 ** -40),
                                  R.rec_bound(n_b, eP_b), R.rec_bound(n_f, eP_f), ptr(sexp), ptr(delta)))
    s_got, d_got = host(sexp), host(delta)
    want, norms = ref_scales(W, nrows, n_b, bK, 1, 0)
    eq(s_got, want)
    assert np.isnan(d_got[rows256:]).all()
    eq(d_got[nrows:rows256], 0.0)
    assert d_got[20] == 0.0 and all(np.isposinf(d_got[i]) for i in (21, 22, 23))       # zero row: 0; non-finite / overflowing norm: +Inf
    worst = 0.0
    for i in range(nrows):
        k = kinds.get(i)
        if k in ("zero", "nan", "inf", "overflow"):
            continue
        assert np.isfinite(d_got[i]) and d_got[i] > 0.0
        if isinstance(k, tuple) and abs(k[1]) > 900:
            continue        # the fp64 terms of δ under- or overflow out there, and the restatement knows no clamp: finite and positive is all that is claimed
        l1, mx = norms[i]
        s, d = R.guard_delta(l1, mx, i, sf2, n_b, rows256)
        assert s == want[i]
        # the kernel evaluates the expression on L1·(1 + (i+1)·2^-52) — at most (1 + (i+1)·2^-52) above — and closes with 1 + 2^-40, which
        # its comment allows for fewer than 32 roundings (≤ 2^-48): within [d, d·(1 + (i+1)·2^-52)·(1 + 2^-40)·(1 + 2^-47)]
        g = Fraction(float(d_got[i]))
        assert d <= g <= d * (1 + (i + 1) * R.pow2(-52)) * (1 + R.pow2(-40)) * (1 + R.pow2(-47)), (i, k)
        worst = max(worst, float(g / d - 1))
    check("oz_family/guard_delta", "max_rel_above_exact", worst, 2.0 ** -39)


def test_rowscale_hook_refuses():
    W = dev(np.zeros((256, 256)))
    s = sent_ints(256)
    L = lib()
    for args in [(256, 256, 7, 1, 0, 53), (300, 256, 14, 1, 0, 53), (256, 200, 14, 1, 0, 53), (256, 256, 14, 0, 0, 53), (256, 256, 14, 4, 901, 53),
                 (256, 256, 14, 1, 0, 54)]:
        nrows, r256, n, kper, ktg, kbits = args
        assert L.abo_test_oz_rowscale(0, ptr(W), 256, nrows, r256, n, kper, ktg, kbits, 0, 0, 0, 0.0, 0.0, 0.0, ptr(s), None) == ABO_EINVAL, args
        assert "abo_test_oz_rowscale" in abo._lib.last_error()
    eq(host(s), np.full(256, SENT32))


# ---- (b) the quantiser ---------------------------------------------------------------------------------------------------------------------
def run_quant(x, rows_out, cols_out, ld, n, lower=0, srow=None, sconst=0, kper=1, ktg=0, rmode=0, rper=1, rtg=0, r0=0, rpts=1, rows_in=None,
              cols_in=None, expect=abo._lib.ABO_OK):
    rows_in = x.shape[0] if rows_in is None else rows_in
    cols_in = x.shape[1] if cols_in is None else cols_in
    plane = rows_out * ld
    out, bad = sent_bytes(n * plane + 64), dev(np.zeros(rows_out + 4, dtype=np.int32))
    xd = dev(x)
    sd = dev(np.asarray(srow, dtype=np.int32)) if srow is not None else None
    a = AboTestOzQuantArgs(in_=ptr(xd), ldin=x.shape[1], rows_in=rows_in, cols_in=cols_in, rows_out=rows_out, cols_out=cols_out, lower=lower,
                           sconst=sconst, srow=ptr(sd), kper=kper, ktg=ktg, rmode=rmode, rper=rper, rtg=rtg, nmod=n, r0=r0, rpts=rpts,
                           out=ptr(out), ld=ld, plane=plane, bad=ptr(bad))
    st = lib().abo_test_oz_quant(0, C.byref(a))
    assert st == expect, abo._lib.last_error()
    o = host(out)
    eq(o[n * plane:].view(np.uint8), np.full(64, SENT, dtype=np.uint8))
    return o[:n * plane].reshape(n, plane), host(bad)


def ref_quant(x, rows_in, cols_in, rows_out, cols_out, n, lower, srow, sconst, kper, ktg, rmode, rper, rtg, r0, rpts):
    """(planes [n][rows_out][cols_out], bad rows): residues(rint(x·2^s)) in integers; rows holding a value not below 1e300, or carrying the
    flagged scale, are bad and their bytes unspecified (returned as zeros, masked by the caller)"""
    r = np.arange(rows_in)
    outp = (r0 + r) % rper if rmode == 1 else (r0 + r) // rpts if rmode == 2 else np.zeros(rows_in, dtype=np.int64)
    s = (np.asarray(srow[:rows_in], dtype=np.int64) if srow is not None else np.full(rows_in, sconst, dtype=np.int64)) + np.where(outp != 0, rtg, 0)
    k = np.arange(cols_in)
    e = s[:, None] + np.where((kper > 1) & (k % kper != 0), ktg, 0)[None, :]
    v = np.array(x[:rows_in, :cols_in], dtype=np.float64)
    live = np.ones_like(v, dtype=bool) if not lower else (k[None, :] <= r[:, None])
    v = np.where(live, v, 0.0)
    bad = ~(np.abs(v) < 1e300).all(axis=1)
    if srow is not None:
        bad |= np.asarray(srow[:rows_in]) == R.SEXP_BAD
    v[bad] = 0.0
    xi = np.rint(np.ldexp(v, np.where(bad[:, None], 0, e).astype(np.int32))).astype(np.int64)
    assert np.abs(xi).max() <= 2 ** 52
    planes = np.zeros((n, rows_out, cols_out), dtype=np.int8)
    for l, p in enumerate(R.plan(n)["p"]):
        planes[l, :rows_in, :cols_in] = R.residues(xi, p)
    return planes, bad


def special_integers(n, count, rng):
    """integers the quantiser must get right: ±(2^52 − 1), ±2^52, multiples of every modulus ± (p−1)/2 and ± p/2 for 256, random 52-bit"""
    v = [2 ** 52 - 1, -(2 ** 52 - 1), 2 ** 52, -(2 ** 52), 0, 1, -1, 127, 128, 129, -127, -128, -129, 2 ** 26, 2 ** 26 - 1, -(2 ** 26)]
    for p in R.plan(n)["p"]:
        for m in (1, -1, 12345, -(2 ** 40) // p, (2 ** 51) // p):
            v += [m * p + (p - 1) // 2, m * p - (p - 1) // 2, m * p + p // 2, m * p - p // 2 - 1]
    v = np.array(v, dtype=np.int64)
    out = rng.integers(-2 ** 52, 2 ** 52, count)
    out[rng.permutation(count)[:v.size]] = v
    return out


def compare_planes(got, want, bad_rows, rows_out, cols_out, ld, n):
    for l in range(n):
        full = R.plane_unpack(got[l], rows_out, ld, ld)
        g = full[:, :cols_out].copy()
        g[bad_rows] = 0
        eq(g, want[l], err_msg=f"plane {l}")
        eq(full[:, cols_out:].view(np.uint8), SENT)                         # bytes beyond cols_out of a wider stride: not written


@pytest.mark.parametrize("n", [8, 14, 16])
def test_quantiser_lower_triangular_with_row_scales(n):
    """W's path: lower = 1 (what lies above the diagonal is NOT READ: NaNs there must neither flag nor show), per-row scales of both
    signs, rows_in < rows_out and cols_in no multiple of 16 (zero fill), kper / ktg, the norm ladder of (a) through its own scales, and
    a NaN, an Inf, a 1e300 and a flagged-scale row — bad[r] there and nowhere else."""
    rng = np.random.default_rng(n)
    rows_in, cols_in, rows_out, cols_out, ld = 300, 300, 512, 512, 512
    srow = rng.integers(-30, 61, rows_out)
    kper, ktg = 4, 3
    ints = special_integers(n, rows_in * cols_in, rng).reshape(rows_in, cols_in)
    k = np.arange(cols_in)
    e = srow[:rows_in, None] + np.where(k % kper != 0, ktg, 0)[None, :]
    x = np.ldexp(ints.astype(np.float64), -e.astype(np.int32))               # exact: x·2^s is the chosen integer
    x[5, :6] = np.ldexp(np.array([1, 3, 5, -1, -3, 7]) + 0.0, -1 - e[5, :6].astype(np.int32)) * 1.0      # half-integers: ties to even
    x[6, :3] = [-0.0, 0.0, -0.0]
    x[np.triu_indices(rows_in, 1)] = NAN                                      # above the diagonal: never read
    W, kinds = rowscale_matrix()
    eP = R.plan(n)["eP"]
    for q, i in enumerate(sorted(i for i, kd in kinds.items() if isinstance(kd, tuple))):      # the ladder, through its own scale
        r = 150 + q
        x[r, :r + 1] = 0.0
        x[r, :5] = W[i, :5]
        w = np.abs(x[r, :5]) * np.where(np.arange(5) % kper != 0, 2.0 ** ktg, 1.0)
        srow[r] = R.row_scale(math.fsum(w), float(w.max()), eP, 53, ktg)
    x[40, 7], x[41, 0], x[42, 41], srow[43] = NAN, INF, -1e300, R.SEXP_BAD
    got, bad = run_quant(x, rows_out, cols_out, ld, n, lower=1, srow=srow, kper=kper, ktg=ktg)
    want, badw = ref_quant(x, rows_in, cols_in, rows_out, cols_out, n, 1, srow, 0, kper, ktg, 0, 1, 0, 0, 1)
    assert sorted(np.flatnonzero(badw)) == [40, 41, 42, 43]
    eq(bad[:rows_out], np.pad(badw, (0, rows_out - rows_in)).astype(np.int32))
    eq(bad[rows_out:], 0)
    compare_planes(got, want, np.flatnonzero(badw), rows_out, cols_out, ld, n)
    assert np.abs(want[:, 150:150 + len(LADDER)]).sum() > 0


@pytest.mark.parametrize("n,rmode", [(8, 1), (14, 2), (16, 0)])
def test_quantiser_dense_with_one_scale(n, rmode):
    """K_XZ's path: lower = 0, one scale, kper / ktg on the columns and rmode 1 / 2 with r0 ≠ 0 on the rows, rows_in < rows_out, cols_in no
    multiple of 16, and a plane stride (384) wider than cols_out (320): the bytes beyond keep their sentinel"""
    rng = np.random.default_rng(100 + n)
    rows_in, cols_in, rows_out, cols_out, ld = 200, 300, 256, 320, 384
    sconst, kper, ktg, rper, rtg, r0, rpts = 17, 4, -3, 3, -2, 5, 70
    ints = special_integers(n, rows_in * cols_in, rng).reshape(rows_in, cols_in)
    r, k = np.arange(rows_in), np.arange(cols_in)
    outp = (r0 + r) % rper if rmode == 1 else (r0 + r) // rpts if rmode == 2 else np.zeros(rows_in, dtype=np.int64)
    e = sconst + np.where(outp != 0, rtg, 0)[:, None] + np.where(k % kper != 0, ktg, 0)[None, :]
    x = np.ldexp(ints.astype(np.float64), -e.astype(np.int32))
    x[3, :4] = np.ldexp(np.array([1.0, -1.0, 5.0, 9.0]), -1 - e[3, :4].astype(np.int32))
    x[4, :2] = -0.0
    x[10, 299], x[11, 16], x[199, 0] = NAN, -INF, 1e300
    got, bad = run_quant(x, rows_out, cols_out, ld, n, sconst=sconst, kper=kper, ktg=ktg, rmode=rmode, rper=rper, rtg=rtg, r0=r0, rpts=rpts)
    want, badw = ref_quant(x, rows_in, cols_in, rows_out, cols_out, n, 0, None, sconst, kper, ktg, rmode, rper, rtg, r0, rpts)
    assert sorted(np.flatnonzero(badw)) == [10, 11, 199]
    eq(bad[:rows_out], np.pad(badw, (0, rows_out - rows_in)).astype(np.int32))
    compare_planes(got, want, np.flatnonzero(badw), rows_out, cols_out, ld, n)


def test_quant_hook_refuses():
    x = np.zeros((256, 256))
    for kw in [dict(cols_out=250), dict(ld=200), dict(rows_in=300), dict(cols_in=300), dict(sconst=1100), dict(sconst=-1100), dict(n=7),
               dict(sconst=1020, kper=2, ktg=10)]:
        a = dict(rows_out=256, cols_out=256, ld=256, n=14)
        a.update(kw)
        run_quant(x, a.pop("rows_out"), a.pop("cols_out"), a.pop("ld"), a.pop("n"), expect=ABO_EINVAL, **a)
        assert "abo_test_oz_quant" in abo._lib.last_error()


# ---- (c) the epilogue's residue arithmetic -------------------------------------------------------------------------------------------------
def test_mod_pack4_mad_every_modulus():
    rng = np.random.default_rng(3)
    for l, p in enumerate(R.moduli(16)):
        half = (p - 1) // 2
        edge = []
        for m in (0, 1, -1, 2 ** 30 // p - 1, -(2 ** 30 // p) + 1, 4321, -98765):
            edge += [m * p + half, m * p - half, m * p + half + 1, m * p - half - 1, m * p]
        if p == 256:
            edge += [128, -128, 384, 2 ** 30 - 128, -(2 ** 30) + 128]                # x ≡ 128: the byte is −128
        x = np.concatenate([[2 ** 30, -(2 ** 30), 2 ** 30 - 1, -(2 ** 30) + 1], edge, rng.integers(-2 ** 30, 2 ** 30 + 1, 4096)]).astype(np.int32)
        x = x[:x.size // 4 * 4]
        packed, xd = sent_ints(x.size // 4 + 4), dev(x)
        ok(lib().abo_test_oz_modpack(0, ptr(xd), x.size // 4, l, ptr(packed)))
        got = host(packed)
        eq(got[x.size // 4:], np.full(4, SENT32))
        eq(got[:x.size // 4].view(np.int8), R.residues(x.astype(np.int64), p), err_msg=f"p = {p}")
    assert lib().abo_test_oz_modpack(0, ptr(packed), 1, 16, ptr(packed)) == ABO_EINVAL


# ---- (d) the residue GEMM ------------------------------------------------------------------------------------------------------------------
def gemm_operands(fill, Ti, Tj, n, rng, rows=None):
    """(W [n][rows][Np256] lower-triangular int8, K [n][Mc256][Np256] int8)"""
    Np, Mc = 256 * Ti, 256 * Tj
    rows = Np if rows is None else rows
    tri = np.tril(np.ones((rows, Np), dtype=bool))
    if fill == "m128":
        W = np.where(tri, -128, 0).astype(np.int8)[None].repeat(n, 0)
        K = np.full((n, Mc, Np), -128, dtype=np.int8)
        return W, K
    K = rng.integers(-128, 128, (n, Mc, Np), dtype=np.int8)
    W = rng.integers(-128, 128, (n, rows, Np), dtype=np.int8)
    i, k = np.arange(rows)[:, None], np.arange(Np)[None, :]
    if fill == "random":
        keep = tri
    elif fill == "diag":                    # the last byte of every row's range: a unit skipped early or a shifted slot loses exactly it
        keep = i == k
    elif fill == "edges":                   # the first byte of the row's last half-stage, and column 0
        keep = (k == (i // 64) * 64) | (k == 0)
    elif fill == "k_sparse":                # K non-zero in a single k per half-stage
        keep = tri
        K = np.where((np.arange(Np)[None, None, :] % 64) == (np.arange(Mc)[None, :, None] * 7) % 64, K, 0).astype(np.int8)
    W = np.where(keep[None], W, 0).astype(np.int8)
    return W, K


def ref_u(W, K, n):
    """U [n][rows][Mc]: per-modulus float64 products — exact, every sum below 2^53 — and the nearest residue"""
    ps = R.moduli(n)
    out = np.empty((n, W.shape[1], K.shape[1]), dtype=np.int8)
    for l in range(n):
        c = W[l].astype(np.float64) @ K[l].astype(np.float64).T
        out[l] = R.residues(c.astype(np.int64), ps[l])
    return out


def run_gemm(W, K, Ti, Tj, n, rblocks=0, launches=1, w_wide=False):
    Np, Mc = 256 * Ti, 256 * Tj
    rows = W.shape[1]
    TiU = rows // 256
    # W's planes: rows × Np256 bytes each; with a short view (rblocks) the bytes k ≥ rows of a row are never read: they hold the sentinel
    Wp = np.concatenate([R.plane_pack(np.where(np.arange(Np)[None, :] < rows, W[l], SENT) if w_wide else W[l], Np) for l in range(n)])
    Kp = np.concatenate([R.plane_pack(K[l], Np) for l in range(n)])
    usz = n * TiU * Tj * 65536
    U, Kd, Wd = sent_bytes(n * Ti * Tj * 65536 + 4096), dev(Kp), dev(Wp)
    ok(lib().abo_test_oz_gemm(0, ptr(Kd), ptr(Wd), Np, Mc, n, rblocks, rows * Np if rblocks else 0, ptr(U), launches))
    u = host(U)
    eq(u[usz:].view(np.uint8), SENT)                                           # blocks beyond the rows covered, and the guard behind U
    return R.u_unpack(u, n, TiU, Tj)


GEMM_SHAPES = [
    (1, 1, 8, ("m128", "random", "diag")),
    (2, 3, 14, ("m128", "random", "diag", "edges", "k_sparse")),
    (3, 9, 14, ("random", "diag", "edges")),              # tjg = 16: padding tickets
    (5, 2, 16, ("m128", "random")),                       # nh = 20: the draw at the tile's start
    (6, 1, 12, ("random", "diag")),                       # nh = 24: the draw inside the loop
    (1, 65, 14, ("random",)),                             # two column groups, the second ragged
]


@pytest.mark.parametrize("Ti,Tj,n,fills", GEMM_SHAPES)
def test_residue_gemm_byte_for_byte(Ti, Tj, n, fills):
    rng = np.random.default_rng(1000 * Ti + 10 * Tj + n)
    for fill in fills:
        W, K = gemm_operands(fill, Ti, Tj, n, rng)
        got = run_gemm(W, K, Ti, Tj, n)
        want = ref_u(W, K, n)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (fill, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("n", [8, 9, 10])
@pytest.mark.parametrize("rblocks", [1, 2])
def test_residue_gemm_on_the_first_row_blocks(n, rblocks):
    """the bound pass's view: planes of W that hold 256·rblocks rows at the full row stride (w_plane = 256·rblocks·Np256), U laid out for
    rblocks row blocks; the blocks of U a full launch would have written beyond keep their sentinel"""
    rng = np.random.default_rng(77 + n + rblocks)
    W, K = gemm_operands("random", 3, 2, n, rng, rows=256 * rblocks)
    got = run_gemm(W, K, 3, 2, n, rblocks=rblocks, w_wide=True)
    eq(got, ref_u(W, K, n))


def test_residue_gemm_second_launch_on_counters_the_reconstruction_reset():
    """launches = 2: GEMM, reconstruction (resets the counters), GEMM again without a memset — production's ctr_clean protocol.  The
    second launch's U started as the sentinel and must equal the reference in every byte: the counters were zero and every tile taken."""
    rng = np.random.default_rng(9)
    W, K = gemm_operands("random", 3, 9, 14, rng)
    got = run_gemm(W, K, 3, 9, 14, launches=2)
    eq(got, ref_u(W, K, 14))


def test_gemm_hook_refuses():
    b = sent_bytes(16)
    for args in [(256, 256, 7, 0, 0, 1), (200, 256, 14, 0, 0, 1), (256, 300, 14, 0, 0, 1), (256, 256, 14, 2, 0, 1), (256, 256, 14, 0, 0, 3),
                 (512, 256, 14, 1, 1000, 1)]:
        Np, Mc, n, rb, wp, la = args
        assert lib().abo_test_oz_gemm(0, ptr(b), ptr(b), Np, Mc, n, rb, wp, ptr(b), la) == ABO_EINVAL, args
        assert "abo_test_oz_gemm" in abo._lib.last_error()
    eq(host(b).view(np.uint8), SENT)


# ---- (e), (f) the reconstructions ----------------------------------------------------------------------------------------------------------
NP_E, MC_E, NVALID_E, SK_E = 256, 128, 203, 5
_CRT = {}


def crt_case(n):
    """one set of integers C [256][128] per plan, their residues laid out as U (Tj = 1: Mc = 128 of a 256 block), row scales of both signs"""
    if n in _CRT:
        return _CRT[n]
    rng = np.random.default_rng(40 + n)
    pl = R.plan(n)
    P, eP = pl["P"], pl["eP"]
    margin = 1 << (eP - 20)
    Cs = np.empty((NP_E, MC_E), dtype=object)
    for i in range(NP_E):
        for j in range(MC_E):
            Cs[i, j] = int(rng.integers(-2 ** 62, 2 ** 62)) * (P // 2 - margin) // 2 ** 62            # full width: (−P/2, P/2) less a margin
    # the engine's contract |C| < P/4 at its ends, small values, and values next to ±P/2 (c1 + c2 next to a multiple of P, still on the
    # side of it that the rounding of Q cannot change: 2^(eP−20) ≫ rec away)
    special = [0, 1, -1, 2 ** eP - 1, -(2 ** eP - 1), P // 2 - margin, -(P // 2 - margin), 2 ** 53 + 1, -(2 ** 53) - 1, 3, -255]
    for q, c in enumerate(special):
        Cs[q % 7, 3 + 9 * q] = c
        Cs[100 + q, q] = c
    sexp = rng.integers(-40, 61, NP_E).astype(np.int32)
    U = np.zeros((n, 256, 256), dtype=np.int8)
    U[:, :, :MC_E] = R.residues_of(Cs, n)
    _CRT[n] = (Cs, sexp, dev(R.u_pack(U)), pl)
    return _CRT[n]


def exact_v(Cs, sexp, sK, extra=None):
    """V = C·2^−(s_i + sK) (·2^extra_j) as exact rationals"""
    out = np.empty(Cs.shape, dtype=object)
    for i in range(Cs.shape[0]):
        f = R.pow2(-(int(sexp[i]) + sK))
        for j in range(Cs.shape[1]):
            out[i, j] = Cs[i, j] * f * (R.pow2(int(extra[j])) if extra is not None else 1)
    return out


@pytest.mark.parametrize("n", [8, 12, 14, 16])
@pytest.mark.parametrize("rmode", [0, 1, 2])
def test_reconstruction_to_v(n, rmode):
    Cs, sexp, Ud, pl = crt_case(n)
    rec = R.rec_bound(n, pl["eP"])
    rper, rtg, r0, rpts = 3, 4, 7, 50
    ldv = NP_E + 6
    sx = sexp.copy()
    # scale extremes: a flagged scale, a factor 2^−(s+sK) below 2^-1074 (was: V = 0, finite and wrong) → NaN rows; a subnormal factor → exact
    sx[60], sx[61], sx[62] = R.SEXP_BAD, 1075 - SK_E, 1070 - SK_E
    bad_row, bad_col = np.zeros(NP_E, dtype=np.int32), np.zeros(256, dtype=np.int32)
    bad_row[17], bad_col[33] = 1, 1
    V = dev(np.full((MC_E + 1, ldv), NAN))
    ctr, sxd, brd, bcd = sent_ints(16), dev(sx), dev(bad_row), dev(bad_col)
    for launch in range(2):
        ok(lib().abo_test_oz_crt(0, ptr(Ud), 1, n, ptr(sxd), SK_E, ptr(brd), ptr(bcd), NP_E, MC_E, NVALID_E, rmode, rper, rtg,
                                 r0, rpts, None, None, 0, ptr(V), ldv, 0, ptr(ctr)))
        eq(host(ctr), np.r_[np.zeros(8, dtype=np.int32), np.full(8, SENT32)])        # the 8 counters zero, also after a second launch
    got = host(V)
    assert np.isnan(got[:, NVALID_E:]).all() and np.isnan(got[MC_E]).all()            # nothing beyond nvalid (203: not a multiple of 8), nothing beyond Mc
    j = np.arange(MC_E)
    outp = (r0 + j) % rper if rmode == 1 else (r0 + j) // rpts if rmode == 2 else np.zeros(MC_E, dtype=np.int64)
    extra = np.where(outp != 0, rtg, 0)
    nanrow = np.zeros(NVALID_E, bool)
    nanrow[[17, 60, 61]] = True
    g = got[:MC_E, :NVALID_E].T                                                          # [i][j]
    nanmask = nanrow[:, None] | (j == 33)[None, :]
    eq(np.isnan(g), nanmask)                                                             # NaN in exactly those rows and that column
    worst, signs = 0.0, 0
    for i in range(NVALID_E):
        sh = int(sx[i]) + SK_E
        for jj in range(MC_E):
            if nanmask[i, jj]:
                continue
            c = Cs[i, jj]
            back = Fraction(float(g[i, jj])) * R.pow2(sh - int(extra[jj]))               # V·2^(s+sK), exact
            bound = rec + abs(c) * 2.0 ** -52
            worst = max(worst, float(abs(back - c)) / bound)
            if abs(c) > 2 * rec:
                assert (g[i, jj] > 0) == (c > 0), (i, jj)                                # the sign, on its own
                signs += 1
            elif c == 0:
                assert abs(back) <= rec
    assert signs > 20000
    check(f"oz_family/crt_v_n{n}_rmode{rmode}", "reached_over_bound", worst, 1.0)


def sums_reference(Cs, sx, n, pl, nvalid, delta=None):
    """(Σ_i d_i², the bar) per 128-row block and candidate in exact rationals: d = v, or max(|v| − δ_i, 0) under a guard.
    bar = Σ_i (2|v_i|e_i + e_i²) + (R + 2)·2^-53·Σ v_i², e_i the bound of (e) scaled, R the rows summed."""
    rec = Fraction(R.rec_bound(n, pl["eP"]))
    want, bar = np.zeros((2, MC_E), dtype=object), np.zeros((2, MC_E), dtype=object)
    for tb in range(2):
        rows = range(128 * tb, min(128 * tb + 128, nvalid))
        for j in range(MC_E):
            s2 = e2 = v2 = Fraction(0)
            for i in rows:
                f = R.pow2(-(int(sx[i]) + SK_E))
                v, e = abs(Cs[i, j]) * f, (rec + abs(Cs[i, j]) * R.pow2(-52)) * f
                d = v if delta is None else (max(v - Fraction(float(delta[i])), 0) if np.isfinite(delta[i]) else Fraction(0))
                s2 += d * d
                v2 += v * v
                e2 += 2 * v * e + e * e
            want[tb, j], bar[tb, j] = s2, e2 + (len(rows) + 2) * R.pow2(-53) * v2
    return want, bar


def run_sums(n, sx, generic, delta=None, Np=NP_E, nvalid=NVALID_E, bad_row=None, Ti=1):
    Cs, _, Ud, pl = crt_case(n)
    part, sxd = dev(np.full((Np // 128 + 1, MC_E + 8), NAN)), dev(sx)
    brd = dev(bad_row) if bad_row is not None else None
    dld = dev(delta) if delta is not None else None
    ok(lib().abo_test_oz_crt(0, ptr(Ud), Ti, n, ptr(sxd), SK_E, ptr(brd), None, Np, MC_E, nvalid,
                             0, 1, 0, 0, 1, ptr(dld), ptr(part), MC_E + 8, None, 0, generic, None))
    got = host(part)
    assert np.isnan(got[:, MC_E:]).all() and np.isnan(got[-1]).all()
    return got[:-1, :MC_E]


def held(case, got, want, bar):
    worst = max(float(abs(Fraction(float(got[t, j])) - want[t, j]) / bar[t, j]) for t in range(got.shape[0]) for j in range(got.shape[1]) if bar[t, j] > 0)
    check(case, "reached_over_bound", worst, 1.0)


@pytest.mark.parametrize("n", [14, 8, 12])
def test_reconstruction_to_sums_every_instantiation(n):
    """<14> and <0> at 14, <0> at 12, and at 8 moduli <0> exact, <8, true> and <0, true>: the compile-time form equals the generic one bit
    for bit; each is held to the bar against exact rational sums"""
    Cs, sexp, Ud, pl = crt_case(n)
    want, bar = sums_reference(Cs, sexp, n, pl, NVALID_E)
    plain = run_sums(n, sexp, 1)
    held(f"oz_family/crt_sums_n{n}", plain, want, bar)
    if n == 14:
        eq(run_sums(n, sexp, 0).view(np.int64), plain.view(np.int64))                    # <14> against <0>
    if n == 8:
        # the guard: δ in {0, just below, equal to, just above |v| of candidate 0, +Inf}, row by row
        v0 = np.array([float(abs(Cs[i, 0]) * R.pow2(-(int(sexp[i]) + SK_E))) for i in range(NP_E)])
        delta = np.where(np.arange(NP_E) % 5 == 0, 0.0, np.where(np.arange(NP_E) % 5 == 1, np.nextafter(v0, 0.0), np.where(
            np.arange(NP_E) % 5 == 2, v0, np.where(np.arange(NP_E) % 5 == 3, np.nextafter(v0, INF), INF))))
        shave = 1.0 - (NVALID_E + 16) * 2.0 ** -52
        g8 = run_sums(n, sexp, 0, delta=delta)                                            # <8, true>
        g0 = run_sums(n, sexp, 1, delta=delta)                                            # <0, true>
        eq(g8.view(np.int64), g0.view(np.int64))
        assert np.all(g8 <= plain)                                                         # never above the exact form's, entry by entry
        wg, _ = sums_reference(Cs, sexp, n, pl, NVALID_E, delta=delta)
        held("oz_family/crt_sums_guarded_n8", g8, wg * Fraction(shave), bar)


def test_reconstruction_to_sums_limits_and_flags():
    n = 14
    Cs, sexp, Ud, pl = crt_case(n)
    base = run_sums(n, sexp, 0)
    # U holds ONE row block (Ti = 1) of a model with Np = 512, nvalid = 400: blocks tb < 2 over min(nvalid, 256) rows, tb ≥ 2 untouched
    sx = np.r_[sexp, np.full(256, 12345, dtype=np.int32)]
    got = run_sums(n, sx, 0, Np=512, nvalid=400)
    assert np.isnan(got[2:]).all()
    want, bar = sums_reference(Cs, sexp, n, pl, 256)
    held("oz_family/crt_sums_rblocks_n14", got[:2], want, bar)
    eq(got[0].view(np.int64), base[0].view(np.int64))
    # a flagged row, and a row whose scaling factor leaves fp64's range, poison their 128-row block only
    bad = np.zeros(NP_E, dtype=np.int32)
    bad[130] = 1
    got = run_sums(n, sexp, 0, bad_row=bad)
    assert np.isnan(got[1]).all()
    eq(got[0].view(np.int64), base[0].view(np.int64))
    for s_bad in (R.SEXP_BAD, 1075 - SK_E, -1024 - SK_E):
        sx = sexp.copy()
        sx[5] = s_bad
        got = run_sums(n, sx, 0)
        assert np.isnan(got[0]).all()
        eq(got[1].view(np.int64), base[1].view(np.int64))


def test_crt_hook_refuses():
    b = sent_bytes(64)
    L = lib()
    P = ptr(b)
    for args in [(1, 7, 256, 128, 100, 0), (0, 14, 256, 128, 100, 0), (1, 14, 200, 128, 100, 0), (1, 14, 256, 100, 100, 0), (1, 14, 256, 128, 300, 0),
                 (1, 14, 256, 128, 100, 2)]:
        Ti, n, Np, Mc, nv, gen = args
        assert L.abo_test_oz_crt(0, P, Ti, n, P, 0, None, None, Np, Mc, nv, 0, 1, 0, 0, 1, None, P, Mc, None, 0, gen, None) == ABO_EINVAL, args
        assert "abo_test_oz_crt" in abo._lib.last_error()
    assert L.abo_test_oz_crt(0, P, 1, 14, P, 0, None, None, 256, 128, 100, 0, 1, 0, 0, 1, P, None, 0, P, 256, 0, None) == ABO_EINVAL      # V with a guard
    assert L.abo_test_oz_crt(0, P, 1, 14, P, 0, None, None, 256, 128, 100, 1, 1, 0, 0, 1, P, P, 128, None, 0, 0, None) == ABO_EINVAL       # a guard with rmode
    eq(host(b).view(np.uint8), SENT)


# ---- (g) the chain ----------------------------------------------------------------------------------------------------------------------------
def test_stages_chained_equal_the_one_call_contraction():
    """(a) → (b) on W → (b) on K_XZ → (d) → (f) through the hooks, on the operands of test_gpu_ozaki's arbitrary-operand case (640, 384,
    600, 14): the final partial equals abo_test_oz_contract's bit for bit — the hooks drive the production path, not a copy of it"""
    import torch
    Np, Mc, nvalid, n = 640, 384, 600, 14
    rng = np.random.default_rng(Np + Mc)
    W = np.tril(rng.standard_normal((Np, Np)) * 10.0 ** rng.uniform(-6, 6, (Np, 1)) * 10.0 ** rng.uniform(-3, 0, (Np, Np)))
    W[nvalid:] = 0.0
    W[:, nvalid:] = 0.0
    W[np.arange(nvalid, Np), np.arange(nvalid, Np)] = 1.0
    kmax = 3.7
    K = rng.uniform(-kmax, kmax, (Mc, Np)) * (rng.random((Mc, Np)) < 0.7)
    K[:, nvalid:] = 0.0
    Wd, Kd = dev(W), dev(K)
    L = lib()
    want = torch.full((Np // 128, Mc), -1.0, dtype=torch.float64).cuda()
    ok(L.abo_test_oz_contract(0, ptr(Wd), Np, Np, nvalid, ptr(Kd), Np, Mc, kmax, n, ptr(want), Mc))
    Np256, Mc256 = 768, 512
    sK = R.k_scale(kmax)
    sexp, bad_row, bad_col = sent_ints(Np256), dev(np.zeros(Np256, dtype=np.int32)), dev(np.zeros(Mc256, dtype=np.int32))
    WR, KR, U = sent_bytes(n * Np256 * Np256), sent_bytes(n * Mc256 * Np256), sent_bytes(n * Mc256 * Np256)
    ok(L.abo_test_oz_rowscale(0, ptr(Wd), Np, nvalid, Np256, n, 1, 0, 53, 0, 0, 0, 0.0, 0.0, 0.0, ptr(sexp), None))
    qa = AboTestOzQuantArgs(in_=ptr(Wd), ldin=Np, rows_in=nvalid, cols_in=Np, rows_out=Np256, cols_out=Np256, lower=1, sconst=0, srow=ptr(sexp),
                            kper=1, ktg=0, rmode=0, rper=1, rtg=0, nmod=n, r0=0, rpts=1, out=ptr(WR), ld=Np256, plane=Np256 * Np256, bad=ptr(bad_row))
    ok(L.abo_test_oz_quant(0, C.byref(qa)))
    qk = AboTestOzQuantArgs(in_=ptr(Kd), ldin=Np, rows_in=Mc, cols_in=Np, rows_out=Mc256, cols_out=Np256, lower=0, sconst=sK, srow=None,
                            kper=1, ktg=0, rmode=0, rper=1, rtg=0, nmod=n, r0=0, rpts=1, out=ptr(KR), ld=Np256, plane=Mc256 * Np256, bad=ptr(bad_col))
    ok(L.abo_test_oz_quant(0, C.byref(qk)))
    ok(L.abo_test_oz_gemm(0, ptr(KR), ptr(WR), Np256, Mc256, n, 0, 0, ptr(U), 1))
    got = torch.full((Np // 128, Mc), -1.0, dtype=torch.float64).cuda()
    ok(L.abo_test_oz_crt(0, ptr(U), Np256 // 256, n, ptr(sexp), sK, ptr(bad_row), ptr(bad_col), Np, Mc, nvalid, 0, 1, 0, 0, 1, None, ptr(got), Mc,
                         None, 0, 0, None))
    eq(host(got).view(np.int64), host(want).view(np.int64))
    # and the intermediates are what the references say: the row scales, and W's residue planes byte for byte
    ws, _ = ref_scales(np.pad(W, ((0, 128), (0, 0))), nvalid, n, 53, 1, 0)
    eq(host(sexp), ws)
    wantW, badw = ref_quant(W, nvalid, Np, Np256, Np256, n, 1, host(sexp), 0, 1, 0, 0, 1, 0, 0, 1)
    assert not badw.any() and not host(bad_row).any() and not host(bad_col).any()
    wr = host(WR).reshape(n, Np256 * Np256)
    for l in range(n):
        eq(R.plane_unpack(wr[l], Np256, Np256, Np256), wantW[l])
