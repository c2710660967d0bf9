"""Direct tests of the factorisation family (csrc/chol.hip and the blocked driver of csrc/api.hip), piece by piece (-m gpu), through
the abo_test_* hooks of the test build: chol_diag_kernel in modes 0, 2 and 3, potf2_pipe_kernel with trsm_stream_kernel, the blocked
chain with the recursive-doubling inverse, trmv_kernel, nlml_terms_kernel and the bordered append.

Method (tests/chol_ref.py).  On the exact family every comparison is an equality: the expected L, L⁻¹ and L⁻ᵀ are known bit for bit.
Every output buffer starts as NaN — an entry a kernel must not write still is NaN afterwards — and inputs carry a finite sentinel
(2⁴⁰) behind their logical width.  Elsewhere (a signed SPD family, kernel matrices of clustered points down to noise 1e-10) the bar is
a backward-error measure set beside LAPACK's on the same matrix:  8 × max(LAPACK's own, 16·2⁻⁵³·kappa16)  — the second term is the
known bound of a solve through explicit 16×16 inverses, the 8 covers the reciprocal multiplies and the 2-ulp pivots — recorded through
parity_record.check under chol/… names.

The a-priori ceiling on the signed family, γ_{n+13}.  Higham's γ_{n+1} (ASNA Thm 10.3) counts, for entry (i, j), the roundings of the
inner sum and two more (the division, the square root).  Here the inner sums are fused multiply-adds, one rounding a term: at most
n − 1.  What replaces the division: an even column is scaled by r0 = (1 + ε0)/√d0, |ε0| ≤ 2u (two coupled Goldschmidt steps leave
(ρ_g − ρ_h)/2 + one rounding, the doubling h + h is exact), so L_ij·L_jj = s_ij·(1 + ε0)²(1 + δ)²: 6 roundings' worth.  An odd column is
scaled by rp1 = fl(fl(d0·r0)·rD), rD = (1 + εD)/√det: L_ij·L_jj = s_ij·(1 + ε0)²(1 + εD)²(1 + δ)⁶, 4 + 4 + 6 = 14.  n − 1 + 14 = n + 13 ≤ n + 16."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import ABO_EINVAL, AboTestAppendArgs
from oracle import gp_oracle as O

from tests import chol_ref as R
from tests import parity_record
from tests.parity_record import check

NAN = float("nan")
INF = float("inf")
eq = np.testing.assert_array_equal          # NaN == NaN at the same position, −0.0 == 0.0
SW, SS, SUPER = 512, 1024, 6144             # the library's own blocking (csrc/abo_state.h: CholBlocking)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return t.data_ptr()


def info_dev(v=0):
    import torch
    return torch.tensor([v], dtype=torch.int64).cuda()


def lib():
    return abo._lib.lib()


def nans(*shape):
    return np.full(shape, NAN)


def embed(rows, ld, r0, B, base=None):
    """a NaN matrix [rows][ld] (or a copy of base) with B at (r0, r0)"""
    M = nans(rows, ld) if base is None else base.copy()
    M[r0:r0 + B.shape[0], r0:r0 + B.shape[1]] = B
    return M


def run3(fn, K, W, WT, *args, info=0):
    """fn(device, K, W, WT, *args, info) on device copies; returns the three matrices and info as the call left them"""
    Kd, Wd, WTd, inf = dev(K), dev(W), dev(WT), info_dev(info)
    abo._lib.check(fn(0, ptr(Kd), ptr(Wd), ptr(WTd), *args, ptr(inf)))
    return host(Kd), host(Wd), host(WTd), int(host(inf)[0])


_CASES = {}


def exact(n):
    if n not in _CASES:
        _CASES[n] = R.exact_case(n, seed=n)
    return _CASES[n]


# ---- a. the diagonal block: modes 0 and 2, potf2_pipe ------------------------------------------------------------------------------------
@pytest.mark.parametrize("r0", [0, 256])
@pytest.mark.parametrize("pad", [0, 128])
def test_diag_block_mode0_exact(r0, pad):
    A, L0, W0 = exact(128)
    ext, ld = r0 + 128, r0 + 128 + pad
    K, W, WT, info = run3(lib().abo_test_chol_diag, embed(ext, ld, r0, A), nans(ext, ld), nans(ext, ld), ld, r0)
    assert info == 0
    eq(K, embed(ext, ld, r0, L0))                   # L₀ with exact zeros above the diagonal; NaN (untouched) around the block
    eq(W, embed(ext, ld, r0, W0))
    eq(WT, embed(ext, ld, r0, W0.T))


@pytest.mark.parametrize("nblocks", [1, 3])
@pytest.mark.parametrize("pad", [0, 128])
def test_trtri_batched_mode2_exact(nblocks, pad):
    n, ld = 128 * nblocks, 128 * nblocks + pad
    K, Ww, WTw = nans(n, ld), nans(n, ld), nans(n, ld)
    for b in range(nblocks):
        _, Lb, Wb = R.exact_case(128, seed=50 + b)
        K, Ww, WTw = embed(n, ld, 128 * b, Lb, K), embed(n, ld, 128 * b, Wb, Ww), embed(n, ld, 128 * b, Wb.T, WTw)
    Ko, W, WT, info = run3(lib().abo_test_trtri_batched, K, nans(n, ld), nans(n, ld), ld, nblocks)
    assert info == 0
    eq(Ko, K)
    eq(W, Ww)
    eq(WT, WTw)


def _pipe_want(ext, ld, r0, W0, zero_rows):
    W, WT = nans(ext, ld), nans(ext, ld)
    if zero_rows:
        for M in (W, WT):
            M[r0:r0 + 128, :r0] = 0.0
            M[r0:r0 + 128, r0 + 128:] = 0.0
    for o in range(0, 128, 16):
        W[r0 + o:r0 + o + 16, r0 + o:r0 + o + 16] = W0[o:o + 16, o:o + 16]
        WT[r0 + o:r0 + o + 16, r0 + o:r0 + o + 16] = W0[o:o + 16, o:o + 16].T
    return W, WT


@pytest.mark.parametrize("r0", [0, 256])
@pytest.mark.parametrize("pad", [0, 128])
@pytest.mark.parametrize("zero_rows", [0, 1])
def test_potf2_pipe_exact(r0, pad, zero_rows):
    """the panel chain's diagonal-block kernel: L₀ to K, the eight 16×16 diagonal sub-blocks of L₀⁻¹ to W / WT and nothing else of the
    128×128 block; with zero_rows the block's rows are zeroed in every column of ld outside it; rows below r0 + 128 exist and stay NaN"""
    A, L0, W0 = exact(128)
    ext, ld = r0 + 128 + 16, r0 + 128 + pad
    K, W, WT, info = run3(lib().abo_test_chol_panel, embed(ext, ld, r0, A), nans(ext, ld), nans(ext, ld), ld, r0, 0, zero_rows)
    assert info == 0
    eq(K, embed(ext, ld, r0, L0))
    Ww, WTw = _pipe_want(ext, ld, r0, W0, zero_rows)
    eq(W, Ww)
    eq(WT, WTw)


# ---- b. failing pivots ---------------------------------------------------------------------------------------------------------------------
def _bad(A, L0, js):
    B = A.copy()
    for j in js:
        B[j, j] -= 2.0 * L0[j, j] ** 2
    return B


def test_failing_pivot_at_every_position_mode0_and_pipe():
    """A[j][j] −= 2·L₀[j][j]²: pivot j is −L₀[j][j]², clearly negative whatever the rounding.  Every j of the block — both parities of
    the pair form, every sub-block, every spine-wave split — in mode 0 (r0 = 0; nothing may be written) and through potf2_pipe at
    r0 = 128: info = r0 + j + 1."""
    import torch
    A, L0, _ = exact(128)
    fn0, fnp = lib().abo_test_chol_diag, lib().abo_test_chol_panel
    nan0 = dev(nans(128, 128))
    for j in range(128):
        B = _bad(A, L0, [j])
        Kd, Wd, WTd, inf = dev(B), nan0.clone(), nan0.clone(), info_dev(0)
        abo._lib.check(fn0(0, ptr(Kd), ptr(Wd), ptr(WTd), 128, 0, ptr(inf)))
        assert int(inf.item()) == j + 1, j
        assert torch.equal(Kd, dev(B)) and bool(torch.isnan(Wd).all()) and bool(torch.isnan(WTd).all()), j
        Kd, Wd, WTd, inf = dev(embed(256, 256, 128, B)), dev(nans(256, 256)), dev(nans(256, 256)), info_dev(0)
        abo._lib.check(fnp(0, ptr(Kd), ptr(Wd), ptr(WTd), 256, 128, 0, 1, ptr(inf)))
        assert int(inf.item()) == 128 + j + 1, j


def _info_of(B, r0=0, pipe=False):
    n = r0 + 128
    if pipe:
        return run3(lib().abo_test_chol_panel, embed(n, n, r0, B), nans(n, n), nans(n, n), n, r0, 0, 0)[3]
    return run3(lib().abo_test_chol_diag, embed(n, n, r0, B), nans(n, n), nans(n, n), n, r0)[3]


@pytest.mark.parametrize("pipe", [False, True])
def test_zero_nan_and_infinite_pivots(pipe):
    """"not a positive normal number" (register_potf2_step_lds): exact zeros at both parities, NaN at both parities, in the first and a
    later sub-block and in the last column; two bad pivots: the lower one.  +Inf passes the compare (it is ≥ 2.3e-308) but has the
    reciprocal square root 0: the pair's columns become NaN and the NEXT pair's pivot fails — a failure is reported, two columns late
    (info = 3 for column 0), as the kernel's comment now states."""
    A, L0, _ = exact(128)
    r0 = 128 if pipe else 0
    B = A.copy(); B[0, 0] = 0.0
    assert _info_of(B, r0, pipe) == r0 + 1
    B = A.copy(); B[1, 1] = L0[1, 0] ** 2                   # a − b²/d0 = 0: a pair determinant that is exactly zero
    assert B[1, 1] * B[0, 0] - B[1, 0] ** 2 == 0.0
    assert _info_of(B, r0, pipe) == r0 + 2
    for j in (0, 1, 17, 127):
        B = A.copy(); B[j, j] = NAN
        assert _info_of(B, r0, pipe) == r0 + j + 1, j
    for js in ((5, 70), (5, 9), (70, 6), (126, 127)):
        assert _info_of(_bad(A, L0, js), r0, pipe) == r0 + min(js) + 1, js
    B = A.copy(); B[0, 0] = INF
    got = _info_of(B, r0, pipe)
    print(f"+Inf at pivot 0 ({'potf2_pipe' if pipe else 'mode 0'}): info = {got}")
    assert got == r0 + 3


def test_a_preset_info_leaves_everything_alone():
    """info = 7 on the way in: mode 0, mode 2, the panel pair and the blocked chain write nothing and leave 7 — except the zeroing
    workgroups of potf2_pipe (zero_rows; the chain of a model of more than one block always asks for them), which run regardless of the
    status word, as the kernel states: rows of W / WT outside the diagonal blocks come back as zeros, the blocks themselves untouched."""
    A, L0, _ = exact(256)
    n = 256
    K0 = A.copy()
    for fn, args in ((lib().abo_test_chol_diag, (n, 128)), (lib().abo_test_trtri_batched, (n, 2)),
                     (lib().abo_test_chol_panel, (n, 0, 128, 0)), (lib().abo_test_chol_blocked, (128, 128, SW, SS, SUPER))):
        Kin = K0[:128, :128].copy() if fn == lib().abo_test_chol_blocked else K0
        m = Kin.shape[0]
        ldk = args[0]
        K, W, WT, info = run3(fn, Kin, nans(m, ldk), nans(m, ldk), *args, info=7)
        assert info == 7
        eq(K, Kin)
        assert np.isnan(W).all() and np.isnan(WT).all()
    zeroed = nans(n, n)
    zeroed[:128, 128:] = 0.0
    K, W, WT, info = run3(lib().abo_test_chol_panel, K0, nans(n, n), nans(n, n), n, 0, 128, 1, info=7)
    assert info == 7
    eq(K, K0); eq(W, zeroed); eq(WT, zeroed)
    zeroed[128:, :128] = 0.0
    K, W, WT, info = run3(lib().abo_test_chol_blocked, K0, nans(n, n), nans(n, n), n, n, SW, SS, SUPER, info=7)
    assert info == 7
    eq(K, K0); eq(W, zeroed); eq(WT, zeroed)


# ---- shared bars -----------------------------------------------------------------------------------------------------------------------------
def _factor_bars(case, A, L, ceiling=None):
    """eta, rho of the library's L against 8 × max(LAPACK's on the same A, 16·2⁻⁵³·kappa16); returns the figures"""
    e, r = R.backward(A, L)
    el, rl = R.backward(A, np.linalg.cholesky(A))
    k16 = R.kappa16(L)
    print(f"{case}: eta {e:.3e} (LAPACK {el:.3e})  rho {r:.3e} (LAPACK {rl:.3e})  kappa16 {k16:.3e}")
    check(case, "eta_lapack", el, INF, tighten=False)
    check(case, "rho_lapack", rl, INF, tighten=False)
    check(case, "kappa16", k16, INF, tighten=False)
    check(case, "eta", e, 8.0 * max(el, R.inv_bar(k16)))
    check(case, "rho", r, 8.0 * max(rl, R.inv_bar(k16)))
    if ceiling is not None:
        assert r <= ceiling, (case, r, ceiling)
    return e, r, el, rl, k16


# ---- c. scale ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [100, -100, 200, -200])
def test_scaled_block_inside_the_supported_range(k):
    """the pair form multiplies two diagonal entries (det = a·d0 − b²): A·4^k must factor to L·2^k with unchanged backward error"""
    A = R.signed_spd(128, seed=1)
    K, W, WT, info = run3(lib().abo_test_chol_diag, np.ldexp(A, 2 * k), nans(128, 128), nans(128, 128), 128, 0)
    assert info == 0
    assert np.isfinite(K).all() and np.isfinite(W).all()
    _factor_bars(f"chol/scale_4^{k}", A, np.ldexp(K, -k), ceiling=R.gamma(128 + 13))
    eq(WT, W.T)


def test_scale_edge_is_recorded():
    """k = ±250: a·d0 ≈ 2^±1000 still normal; ±260: it leaves the range.  What the kernel reports there is recorded (DESIGN.md states the
    supported range of σ_f² from it); nothing is asserted but that the call returns."""
    A = R.signed_spd(128, seed=1)
    for k in (250, -250, 260, -260):
        K, _, _, info = run3(lib().abo_test_chol_diag, np.ldexp(A, 2 * k), nans(128, 128), nans(128, 128), 128, 0)
        print(f"scale 4^{k}: info = {info}, finite = {bool(np.isfinite(K).all())}")
        check("chol/scale_edge", f"info_4^{k}", info, INF, tighten=False)


# ---- d. the panel solve ------------------------------------------------------------------------------------------------------------------
def _panel(Asub, r0, nrows, pad=0):
    """potf2_pipe + trsm_stream on the (128 + nrows)-matrix Asub placed at (r0, r0): only its first 128 columns enter K; returns
    (L_bb, X, the whole K)"""
    m = 128 + nrows
    rows, ld = r0 + m + 16, r0 + 128 + pad
    Kin = nans(rows, ld)
    Kin[r0:r0 + m, r0:r0 + 128] = Asub[:, :128]
    K, W, WT, info = run3(lib().abo_test_chol_panel, Kin, nans(rows, ld), nans(rows, ld), ld, r0, nrows, 0)
    assert info == 0
    return K[r0:r0 + 128, r0:r0 + 128], K[r0 + 128:r0 + m, r0:r0 + 128], K, Kin


@pytest.mark.parametrize("nrows", [16, 128, 400])
@pytest.mark.parametrize("r0", [0, 128])
def test_panel_solve_exact(nrows, r0):
    """X equals the rows of L₀ bit for bit; rows at and below r0 + 128 + nrows, and everything left of column r0, stay NaN"""
    A, L0, _ = exact(128 + nrows)
    Lbb, X, K, Kin = _panel(A, r0, nrows, pad=128 if nrows == 128 else 0)
    want = Kin.copy()
    want[r0:r0 + 128 + nrows, r0:r0 + 128] = L0[:, :128]
    eq(K, want)


def _panel_bars(case, Asub, r0, nrows):
    Lbb, X, _, _ = _panel(Asub, r0, nrows)
    Ap = Asub[128:, :128]
    res = R.panel_res(Ap, X, Lbb)
    ref = R.panel_res(Ap, sla.solve_triangular(Lbb, Ap.T, lower=True).T, Lbb)
    k16 = R.kappa16(Lbb)
    print(f"{case}: residual {res:.3e}  solve_triangular {ref:.3e}  kappa16 {k16:.3e}")
    check(case, "res_lapack", ref, INF, tighten=False)
    check(case, "kappa16", k16, INF, tighten=False)
    check(case, "res", res, 8.0 * max(ref, R.inv_bar(k16)))


@pytest.mark.parametrize("nrows", [16, 128, 400])
@pytest.mark.parametrize("r0", [0, 128])
def test_panel_solve_signed(nrows, r0):
    _panel_bars(f"chol/panel_signed_n{nrows}_r{r0}", R.signed_spd(128 + nrows, seed=nrows), r0, nrows)


@pytest.mark.parametrize("r0", [0, 128])
def test_panel_solve_on_the_ladder(r0):
    for name, A, _ in R.ladder_cases(528):
        _panel_bars(f"chol/panel_{name}_r{r0}", A, r0, 400)


# ---- e. the whole chain ----------------------------------------------------------------------------------------------------------------------
def _blocked(A, Np, ld, blocking=(SW, SS, SUPER)):
    Kin = nans(Np, ld)
    Kin[:, :Np] = A
    K, W, WT, info = run3(lib().abo_test_chol_blocked, Kin, nans(Np, ld), nans(Np, ld), ld, Np, *blocking)
    assert info == 0
    return K, W, WT


@pytest.mark.parametrize("Np,pad,blocking", [(128, 0, (SW, SS, SUPER)), (128, 128, (SW, SS, SUPER)), (256, 0, (SW, SS, SUPER)),
                                             (640, 0, (SW, SS, SUPER)), (640, 128, (SW, SS, SUPER)), (1152, 0, (SW, SS, SUPER)),
                                             (1664, 0, (256, 512, 1024))])
def test_blocked_chain_exact(Np, pad, blocking):
    """L, W = L⁻¹ and WT = Wᵀ equal the known ones, zeros strictly above (below) the diagonal are exact zeros.  1664 rows under
    (256, 512, 1024): one super-strip of two strips, a plain strip behind it, ragged last strips, and the ragged passes of the doubling
    inverse.  The 128-blocks of K strictly above the diagonal are no output: they keep the (symmetric) input.  More than one block:
    the chain zeroes rows < Np of W / WT over all ld columns; one block: only the block is written."""
    A, L0, W0 = exact(Np)
    ld = Np + pad
    K, W, WT = _blocked(A, Np, ld, blocking)
    blk = np.arange(Np) // 128
    upper = blk[:, None] < blk[None, :]
    wantK = nans(Np, ld)
    wantK[:, :Np] = np.where(upper, A, L0)
    eq(K, wantK)
    fill = NAN if Np == 128 else 0.0
    wantW, wantWT = np.full((Np, ld), fill), np.full((Np, ld), fill)
    wantW[:, :Np], wantWT[:, :Np] = W0, W0.T
    eq(W, wantW)
    eq(WT, wantWT)


_LADDER_ROWS = {}


def _chain_bars(case, A, ceiling=None, kap=None):
    n = A.shape[0]
    K, W, WT = _blocked(A, n, n)
    L = np.tril(K)
    e, r, el, rl, k16 = _factor_bars(case, A, L, ceiling)
    eq(WT, W.T)
    eq(np.triu(W, 1), np.zeros((n, n)))
    ir = R.inv_res(L, W)
    Wl, st = sla.lapack.dtrtri(L, lower=1)
    assert st == 0
    irl = R.inv_res(L, np.tril(Wl))
    print(f"{case}: inv_res {ir:.3e} (LAPACK trtri {irl:.3e})")
    check(case, "inv_res_lapack", irl, INF, tighten=False)
    check(case, "inv_res", ir, 8.0 * irl)
    if kap is not None:
        _LADDER_ROWS[case] = (kap, k16, e, el, r, rl, ir, irl)
        os.makedirs(os.path.dirname(parity_record.OUT_PATH), exist_ok=True)
        with open(os.path.join(os.path.dirname(parity_record.OUT_PATH), "chol_backward_error.txt"), "w") as f:
            f.write("# blocked chain at Np = 640 beside LAPACK (potrf / trtri) on the same matrix\n")
            f.write("# case  kappa2(A)  kappa16(L)  eta  eta_lapack  rho  rho_lapack  inv_res  inv_res_lapack\n")
            for c in sorted(_LADDER_ROWS):
                f.write(c + "  " + "  ".join(f"{v:.3e}" for v in _LADDER_ROWS[c]) + "\n")


def test_blocked_chain_signed():
    _chain_bars("chol/chain_signed_640", R.signed_spd(640, seed=640), ceiling=R.gamma(640 + 13))


@pytest.mark.parametrize("fam", R.LADDER_FAMILIES)
@pytest.mark.parametrize("noise", R.NOISES)
def test_blocked_chain_on_the_ladder(fam, noise):
    A = R.ladder_matrix(fam, noise, 640)
    kap = float(np.linalg.cond(A))
    _chain_bars(f"chol/chain_{'se' if fam == O.SE else 'm52'}_noise{noise:.0e}", A, kap=kap)


# ---- f. trmv -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [1, 2, 3, 4, 5, 7, 8, 127, 128, 129, 130, 509, 1027])
@pytest.mark.parametrize("lower", [1, 0])
def test_trmv_exact(Np, lower):
    """integer triangle (zeros in the other one, as the contract states), integer v: the product is exact in any order.  Odd ends of
    the pair loads, the 4-row group tails, one and two trips of the 512-wide unrolled loop; 2⁴⁰ behind column Np of W and behind v[Np)"""
    rng = np.random.default_rng(Np)
    ld = Np + 2 + (Np & 1)
    T = rng.integers(-8, 9, size=(Np, Np)).astype(np.float64)
    T = np.tril(T) if lower else np.triu(T)
    Wm = np.full((Np, ld), R.SENTINEL)
    Wm[:, :Np] = T
    v = np.full(ld, R.SENTINEL)
    v[:Np] = rng.integers(-8, 9, size=Np)
    out = dev(nans(Np + 5))
    Wd, vd = dev(Wm), dev(v)
    abo._lib.check(lib().abo_test_trmv(0, ptr(Wd), ld, ptr(vd), ptr(out), Np, lower))
    want = nans(Np + 5)
    want[:Np] = T @ v[:Np]
    eq(host(out), want)


# ---- g. nlml_terms and the bordered append ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_nlml_terms(N):
    """out[1] = Σ δ_i α_i on integers: an equality.  out[0] = Σ 2·log L_ii against a long double sum: every term carries the device
    log's documented 1 ulp (2⁻⁵² relative; the doubling is exact), a thread adds its ⌈N/256⌉ terms in turn and the tree adds eight
    levels — at most ⌈N/256⌉ + 7 roundings of 2⁻⁵³ each on partial sums bounded by Σ|t_i|; only the diagonal of L is read (the rest is NaN)"""
    rng = np.random.default_rng(N)
    ld = N + 3
    Lm = nans(N, ld)
    dg = rng.uniform(0.5, 3.0, size=N)
    Lm[np.arange(N), np.arange(N)] = dg
    delta, alpha = rng.integers(-8, 9, size=N).astype(np.float64), rng.integers(-8, 9, size=N).astype(np.float64)
    out = dev(nans(4))
    Ld, dd, ad = dev(Lm), dev(delta), dev(alpha)
    abo._lib.check(lib().abo_test_nlml_terms(0, ptr(Ld), ld, ptr(dd), ptr(ad), N, ptr(out)))
    got = host(out)
    assert got[1] == float(np.dot(delta.astype(np.int64), alpha.astype(np.int64)))
    assert np.isnan(got[2:]).all()
    t = 2.0 * np.log(dg.astype(R.LD))
    ref, mag = float(np.sum(t)), float(np.sum(np.abs(t)))
    bar = mag * (2.0 ** -52 + (math.ceil(N / 256) + 7) * 2.0 ** -53) * (1 + 2.0 ** -20)
    print(f"nlml_terms N = {N}: |out[0] − ref| = {abs(got[0] - ref):.3e}, bar {bar:.3e}")
    assert abs(got[0] - ref) <= bar


def _append(N, s2, info0=0):
    import torch
    rng = np.random.default_rng(N)
    cap = N + 6
    ld = cap
    lvec, vvec, krow, aold = (rng.integers(-4, 5, size=N).astype(np.float64) for _ in range(4))
    delta = rng.integers(-8, 9, size=N + 1).astype(np.float64)
    l2 = float(np.dot(lvec.astype(np.int64), lvec.astype(np.int64)))
    kss = l2 + s2
    mats = [torch.full((cap, ld), NAN, dtype=torch.float64, device="cuda") for _ in range(3)]
    anew, vext, scal, inf = dev(nans(cap + 2)), dev(nans(cap + 2)), dev(nans(6)), info_dev(info0)
    keep = [dev(x) for x in (krow, lvec, vvec, aold, delta)]
    a = AboTestAppendArgs(L=ptr(mats[0]), W=ptr(mats[1]), WT=ptr(mats[2]), ld=ld, krow=ptr(keep[0]), lvec=ptr(keep[1]), vvec=ptr(keep[2]),
                          alpha_old=ptr(keep[3]), alpha_new=ptr(anew), vext=ptr(vext), delta=ptr(keep[4]), N=N, cap=cap, kss=kss,
                          scal=ptr(scal), info=ptr(inf))
    abo._lib.check(lib().abo_test_append(0, C.byref(a)))
    return dict(N=N, cap=cap, lvec=lvec, vvec=vvec, krow=krow, aold=aold, delta=delta, mats=mats, anew=host(anew), vext=host(vext),
                scal=host(scal), info=int(inf.item()))


@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 2500])
def test_append_exact(N):
    """integer data and s2 = kss − ‖l‖² a power of four: l_nn, 1/l_nn, β and every output are exact"""
    import torch
    s2 = 16.0
    r = _append(N, s2)
    cap = r["cap"]
    ka = float(np.dot(r["krow"].astype(np.int64), r["aold"].astype(np.int64)))
    beta = (r["delta"][N] - ka) / s2
    assert r["info"] == 0
    eq(r["scal"], np.array([s2, beta, 4.0, ka, NAN, NAN]))
    Lm, Wm, WTm = r["mats"]
    w = -r["vvec"] * 0.25
    rowL, rowW, colWT = nans(cap), nans(cap), nans(cap)
    rowL[:N], rowL[N] = r["lvec"], 4.0
    rowW[:N], rowW[N] = w, 0.25
    colWT[:N], colWT[N] = w, 0.25
    eq(host(Lm[N]), rowL)
    eq(host(Wm[N]), rowW)
    eq(host(WTm[:, N]), colWT)
    # nothing but row N of L and W and column N of WT was written
    assert int((~torch.isnan(Lm)).sum()) == N + 1 and int((~torch.isnan(Wm)).sum()) == N + 1 and int((~torch.isnan(WTm)).sum()) == N + 1
    anew, vext = nans(cap + 2), nans(cap + 2)
    anew[:cap], vext[:cap] = 0.0, 0.0
    anew[:N], anew[N] = r["aold"] - beta * r["vvec"], beta
    vext[:N], vext[N] = -r["vvec"], 1.0
    eq(r["anew"], anew)
    eq(r["vext"], vext)


@pytest.mark.parametrize("s2", [0.0, -1.0, NAN])
def test_append_failing_pivot(s2):
    """s2 not positive: info = N + 1 only if it was 0, a preset info survives, and the write kernel leaves every NaN output NaN"""
    import torch
    for N in (1, 1025):
        for info0 in (0, 5):
            r = _append(N, s2, info0)
            assert r["info"] == (N + 1 if info0 == 0 else 5)
            eq(r["scal"][0], s2)
            assert np.isnan(r["scal"][1:]).all() and np.isnan(r["anew"]).all() and np.isnan(r["vext"]).all()
            assert all(bool(torch.isnan(m).all()) for m in r["mats"])


# ---- h. mode 3 against mode 0 ------------------------------------------------------------------------------------------------------------
_FITS = {}


def _fit_both(N, d):
    """(L, α, L⁻¹) of one model fitted at capacity 128 (the whole fit in one launch: mode 3) and with spare capacity (kernel matrix,
    mode 0 of the diagonal-block kernel, the two mat-vecs), and its centred targets"""
    if (N, d) not in _FITS:
        from abstractbayesopt.jl_amd import synth
        X = synth.points(7, N, d)
        y = synth.objective(X)

        def fit(n_max):
            gp = abo.HipStandardGP(1.3 * abo.with_lengthscale(abo.Matern52Kernel(), 0.7), 1e-3, mean=abo.ConstMean(0.1), n_max=n_max)
            return abo.get_factor(abo.update(gp, X, y))
        _FITS[(N, d)] = (fit(0), fit(256), y - 0.1)
    return _FITS[(N, d)]


MODE3_CASES = [(5, 2), (50, 16), (128, 3)]


@pytest.mark.parametrize("N,d", MODE3_CASES)
def test_one_launch_fit_factor_against_the_mode0_path(N, d):
    """the kernel's comment claims the same bits for the kernel matrix generated into LDS and for the shortened sub-block sweep:
    L and L⁻¹ of the two paths are equal bit for bit"""
    (L3, _, W3), (L0, _, W0), _ = _fit_both(N, d)
    eq(L3, L0)
    eq(W3, W0)


@pytest.mark.parametrize("N,d", MODE3_CASES)
def test_one_launch_fit_alpha_against_the_mode0_path(N, d):
    """α bit for bit: mode 3 forms α = L⁻ᵀ(L⁻¹δ) in trmv_kernel's order of summation (a wave per row, pairs per lane, the xor tree),
    so a model's α does not depend on the path that fitted it.  (Before this test existed mode 3 summed one thread a row in index
    order, and the two paths differed by up to 2.0e-13 at N = 128.)"""
    (_, a3, _), (_, a0, _), _ = _fit_both(N, d)
    eq(a3, a0)


def test_hooks_refuse_what_the_launchers_cannot_take():
    z = info_dev(0)
    p = ptr(z)
    L = lib()
    assert L.abo_test_chol_diag(0, None, p, p, 128, 0, p) == ABO_EINVAL
    assert L.abo_test_chol_diag(0, p, p, p, 128, 128, p) == ABO_EINVAL
    assert L.abo_test_chol_panel(0, p, p, p, 128, 0, 8, 0, p) == ABO_EINVAL          # nrows no multiple of 16
    assert L.abo_test_chol_panel(0, p, p, p, 130, 0, 16, 0, p) == ABO_EINVAL         # ld no multiple of 128
    assert L.abo_test_trtri_batched(0, p, p, p, 128, 2, p) == ABO_EINVAL
    assert L.abo_test_chol_blocked(0, p, p, p, 256, 256, 100, 512, 0, p) == ABO_EINVAL
    assert L.abo_test_chol_blocked(0, p, p, p, 256, 256, 256, 384, 0, p) == ABO_EINVAL   # ss no multiple of sw
    assert L.abo_test_trmv(0, p, 5, p, p, 4, 1) == ABO_EINVAL                         # odd ld
    assert L.abo_test_nlml_terms(0, p, 4, p, p, 0, p) == ABO_EINVAL
    assert L.abo_test_append(0, None) == ABO_EINVAL
