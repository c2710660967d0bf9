"""Direct tests of the fp64 MFMA GEMM family (csrc/gemm.hip), kernel by kernel and mode by mode (-m gpu), through the abo_test_* hooks
of the test build: gemm_nt_kernel (2-D, swizzled and split-k launches), gemm_nt_small_kernel, gemm_skinny_kernel<1..4>,
qei_passd_kernel<1..4>, splitk_reduce_kernel, var_gemm_kernel and var_gemm256s_kernel.

Method (tests/gemm_family_ref.py): operands are integer-valued fp64 small enough that every product and every partial sum is exact in
any summation order, so the reference is a plain numpy product and EVERY comparison is an equality — there is no tolerance in this
file.  Operands are dense (non-zero outside any triangle a mode assumes), rows are padded with a large sentinel behind their logical
width, and every output starts as NaN: an element a kernel should not have written still is NaN afterwards, an element it should have
written no longer is, and a k range that is one block too wide or too narrow changes integers.  The reference of a triangular kmode is
the kernels' stated contract at 128-block granularity (gemm_family_ref.krange)."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import (ABO_EINVAL, GEMM_PATH_SKINNY, GEMM_PATH_SMALL, GEMM_PATH_SPLITK, GEMM_PATH_SWIZZLED,
                                          GEMM_PATH_TILED)

from tests import gemm_family_ref as R
from tests.gemm_family_ref import K_A_LOWER, K_A_UPPER, K_B_LOWER, K_B_UPPER, K_FULL

NAN = float("nan")
eq = np.testing.assert_array_equal          # NaN == NaN at the same position, −0.0 == 0.0 (alpha = 0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return t.data_ptr() if t is not None else None


def gemm(A, B, Cm, Ct=None, *, M, N, K, lda, ldb, ldc, ldct=0, sA=0, sB=0, sC=0, sCt=0, kmode=K_FULL, lower_only=0, batch=1, alpha=1.0,
         beta=0.0, ksplit=0, mrows=0, info=None, offs=(0, 0, 0, 0)):
    """abo_test_gemm_args on device tensors (offs: element offsets of A, B, C, Ct into their tensors); returns the path that ran"""
    import torch
    path = C.c_int32(-99)
    torch.cuda.synchronize()
    es = 8
    st = abo._lib.lib().abo_test_gemm_args(0, ptr(A) + es * offs[0], ptr(B) + es * offs[1], ptr(Cm) + es * offs[2],
                                           ptr(Ct) + es * offs[3] if Ct is not None else None, lda, ldb, ldc, ldct, sA, sB, sC, sCt, M, N, K,
                                           kmode, lower_only, batch, alpha, beta, ksplit, mrows, ptr(info), C.byref(path))
    abo._lib.check(st)
    return path.value


# ---- gemm_nt_kernel / gemm_nt_small_kernel: kmode × lower_only × beta × Ct ----------------------------------------------------------
def _gemm_case(rng, M, N, K):
    lda, ldb = K + 6, K + 2
    A = R.padded(rng, M, K, lda, 64)
    B = R.padded(rng, N, K, ldb, 64)
    C0 = R.ints(rng, (M, N), 64)
    return A, B, C0, {km: R.acc_ref(A, B, M, N, K, km) for km in range(5)}


def _run_modes(monkeypatch, M, N, K, small_env, want_path, seed):
    """every kmode × lower_only × (beta = 0, beta ≠ 0) × (Ct absent, present) of one shape; alpha and beta walk through their sets"""
    rng = np.random.default_rng(seed)
    A, B, C0, acc = _gemm_case(rng, M, N, K)
    Ad, Bd = dev(A), dev(B)
    ldc, ldct = N + 3, M + 5
    low = R.lower_mask(M, N)
    monkeypatch.setenv("ABO_GEMM_SMALL", small_env)
    for n, (kmode, lower_only, has_beta, has_ct) in enumerate(itertools.product(range(5), (0, 1), (0, 1), (0, 1))):
        alpha = R.ALPHAS[n % len(R.ALPHAS)]
        beta = R.BETAS[(n // 2) % len(R.BETAS)] if has_beta else 0.0
        written = low if lower_only else np.ones((M, N), dtype=bool)
        # C on the way in: integers where the kernel reads it (beta ≠ 0, written tiles), NaN everywhere else
        Cin = np.full((M, ldc), NAN)
        if has_beta:
            Cin[:, :N][written] = C0[written]
        val = alpha * acc[kmode] + (beta * C0 if has_beta else 0.0)
        want = np.full((M, ldc), NAN)
        want[:, :N][written] = val[written]
        want_t = np.full((N, ldct), NAN)
        want_t[:, :M][written.T] = val.T[written.T]
        Cd = dev(Cin)
        Ctd = dev(np.full((N, ldct), NAN)) if has_ct else None
        path = gemm(Ad, Bd, Cd, Ctd, M=M, N=N, K=K, lda=K + 6, ldb=K + 2, ldc=ldc, ldct=ldct if has_ct else 0, kmode=kmode,
                    lower_only=lower_only, alpha=alpha, beta=beta)
        what = f"kmode={kmode} lower_only={lower_only} alpha={alpha} beta={beta} ct={has_ct}"
        assert path == want_path, what
        eq(host(Cd), want, err_msg=what)
        if has_ct:
            eq(host(Ctd), want_t, err_msg=what + " (Ct)")


SHAPES = [(384, 256, 384), (256, 384, 256), (128, 128, 128)]


@pytest.mark.parametrize("small_env,want_path", [("0", GEMM_PATH_TILED), ("1", GEMM_PATH_SMALL)])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_every_mode_of_the_tiled_and_the_small_kernel(monkeypatch, M, N, K, small_env, want_path):
    """M > N leaves tiles above the diagonal of a lower_only launch with Tm ≠ Tn untouched (NaN), M < N has k ranges clipped to K"""
    _run_modes(monkeypatch, M, N, K, small_env, want_path, seed=M + N + K)


@pytest.mark.parametrize("small_env", ["0", "1"])
@pytest.mark.parametrize("K", [16, 32, 48, 272])
def test_every_mode_of_the_tiled_kernel_at_short_and_ragged_k(monkeypatch, K, small_env):
    """nk = 1, 2, 3 stages (the pipeline's prologue and its two plain tail stages alone) and K = 272 (steady-state iterations, K no
    multiple of 128, triangular ranges clipped to it): the tiled kernel whatever ABO_GEMM_SMALL says (the small one needs K % 128 = 0)"""
    _run_modes(monkeypatch, 384, 256, K, small_env, GEMM_PATH_TILED, seed=1000 + K)
    _run_modes(monkeypatch, 256, 384, K, small_env, GEMM_PATH_TILED, seed=2000 + K)


def test_default_rule_takes_the_small_kernel_below_65_tiles(monkeypatch):
    monkeypatch.delenv("ABO_GEMM_SMALL", raising=False)
    rng = np.random.default_rng(5)
    A, B, _, acc = _gemm_case(rng, 256, 384, 256)
    Cd = dev(np.full((256, 384), NAN))
    assert gemm(dev(A), dev(B), Cd, M=256, N=384, K=256, lda=262, ldb=258, ldc=384, kmode=K_B_UPPER) == GEMM_PATH_SMALL
    eq(host(Cd), acc[K_B_UPPER])


# ---- batches: the two products of a level of the blocked inverse (api.hip: factorise) ------------------------------------------------
@pytest.mark.parametrize("small_env,want_path", [("0", GEMM_PATH_TILED), ("1", GEMM_PATH_SMALL)])
def test_batched_products_of_the_blocked_inverse(monkeypatch, small_env, want_path):
    """Three batches whose operands are sz×sz blocks of ONE matrix, bstride = 2·sz·(ld + 1) apart (no multiple of the block size, nothing
    overlaps): Tt[b] = WT11[b]·L21[b]ᵀ under K_A_UPPER into a dense batch array, then W21[b] = −W22[b]·Tt[b]ᵀ under K_A_LOWER back into
    the big matrix with its transposed copy in a second one.  Everything outside the operand blocks is NaN: a stride or a range that is
    off reads it."""
    monkeypatch.setenv("ABO_GEMM_SMALL", small_env)
    rng = np.random.default_rng(77)
    sz, nb = 256, 3
    two = 2 * sz
    n = nb * two
    ld = n + 8
    bstride = two * (ld + 1)
    WT, Kmat, W = (np.full((n, ld), NAN) for _ in range(3))
    for b in range(nb):
        r1, r2 = b * two, b * two + sz
        WT[r1:r1 + sz, r1:r1 + sz] = R.ints(rng, (sz, sz), 64)
        Kmat[r2:r2 + sz, r1:r1 + sz] = R.ints(rng, (sz, sz), 64)
        W[r2:r2 + sz, r2:r2 + sz] = R.ints(rng, (sz, sz), 64)
    WTd, Kd, Wd = dev(WT), dev(Kmat), dev(W)
    Tp = dev(np.full((nb, sz, sz), NAN))
    # Tt[j][i] = Σ_{k ≥ 128·(j/128)} WT11[j][k]·L21[i][k]
    p1 = gemm(WTd, Kd, Tp, M=sz, N=sz, K=sz, lda=ld, ldb=ld, ldc=sz, sA=bstride, sB=bstride, sC=sz * sz, kmode=K_A_UPPER, batch=nb,
              offs=(0, sz * ld, 0, 0))
    assert p1 == want_path
    Tt = np.stack([R.acc_ref(WT[b * two:, b * two:], Kmat[b * two + sz:, b * two:], sz, sz, sz, K_A_UPPER) for b in range(nb)])
    eq(host(Tp), Tt)
    # W21[i][j] = −Σ_{k < 128·(i/128 + 1)} W22[i][k]·Tt[j][k], and its transpose into WT's (r1, r2) block
    WTout = dev(np.full((n, ld), NAN))
    p2 = gemm(Wd, Tp, Wd, WTout, M=sz, N=sz, K=sz, lda=ld, ldb=sz, ldc=ld, ldct=ld, sA=bstride, sB=sz * sz, sC=bstride, sCt=bstride,
              kmode=K_A_LOWER, batch=nb, alpha=-1.0, offs=(sz * ld + sz, 0, sz * ld, sz))
    assert p2 == want_path
    want_w, want_wt = W.copy(), np.full((n, ld), NAN)
    for b in range(nb):
        r1, r2 = b * two, b * two + sz
        w21 = -R.acc_ref(W[r2:, r2:], Tt[b], sz, sz, sz, K_A_LOWER)
        want_w[r2:r2 + sz, r1:r1 + sz] = w21
        want_wt[r1:r1 + sz, r2:r2 + sz] = w21.T
    eq(host(Wd), want_w)
    eq(host(WTout), want_wt)


# ---- the info early exit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tiled", "small", "splitk", "skinny"])
def test_info_early_exit(monkeypatch, form):
    """*info = 7 (a failed factorisation): nothing is written; *info = 0: the result of a launch without info"""
    monkeypatch.setenv("ABO_GEMM_SMALL", "1" if form == "small" else "0")
    rng = np.random.default_rng(11)
    M, N, K = 128, 384, 384
    A, B, _, acc = _gemm_case(rng, M, N, K)
    Ad, Bd = dev(A), dev(B)
    kw = dict(M=M, N=N, K=K, lda=K + 6, ldb=K + 2, ldc=N + 2, kmode=K_B_LOWER, alpha=-1.5)
    nz = 1
    if form in ("splitk", "skinny"):
        nz = 3
        kw.update(ksplit=128, sC=M * (N + 2), mrows=32 if form == "skinny" else 0)
    want_path = {"tiled": GEMM_PATH_TILED, "small": GEMM_PATH_SMALL, "splitk": GEMM_PATH_SPLITK, "skinny": GEMM_PATH_SKINNY}[form]
    out = {}
    for tag, info in (("none", None), ("zero", dev(np.array([0], dtype=np.int64))), ("seven", dev(np.array([7], dtype=np.int64)))):
        Cd = dev(np.full((nz, M, N + 2), NAN))
        Ctd = dev(np.full((N, M), NAN)) if nz == 1 else None
        assert gemm(Ad, Bd, Cd, Ctd, ldct=M if nz == 1 else 0, info=info, **kw) == want_path
        out[tag] = host(Cd)
        if tag == "seven":
            assert np.isnan(out[tag]).all()
            assert Ctd is None or np.isnan(host(Ctd)).all()
    assert not np.isnan(out["none"][:, :32, :N]).all()
    eq(out["zero"], out["none"])
    if nz == 1:
        eq(out["none"][0][:, :N], -1.5 * acc[K_B_LOWER])


# ---- the swizzled launch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [16, 17, 18, 19])
def test_swizzled_syrk_updates_every_lower_tile_exactly_once(monkeypatch, T):
    """C −= A·Aᵀ on the lower tiles of a T×T tile grid through the 1-D XCD-aware launch: last super-rows of 0, 1, 2 and 3 tile rows.  A
    tile the map misses keeps its C, a tile hit twice loses A·Aᵀ twice; the tiles above the diagonal stay NaN; same result as the 2-D
    launch."""
    monkeypatch.delenv("ABO_GEMM_SMALL", raising=False)
    monkeypatch.delenv("ABO_GEMM_NO_SWIZZLE", raising=False)
    rng = np.random.default_rng(T)
    n, K = 128 * T, 32
    lda, ldc = K + 8, n + 2
    A = R.padded(rng, n, K, lda, 64)
    low = R.lower_mask(n, n)
    Cin = np.full((n, ldc), NAN)
    Cin[:, :n][low] = R.ints(rng, (n, n), 64)[low]
    want = Cin.copy()
    want[:, :n][low] -= (A[:, :K] @ A[:, :K].T)[low]
    Ad = dev(A)
    kw = dict(M=n, N=n, K=K, lda=lda, ldb=lda, ldc=ldc, lower_only=1, alpha=-1.0, beta=1.0)
    Cs = dev(Cin)
    assert gemm(Ad, Ad, Cs, **kw) == GEMM_PATH_SWIZZLED
    got = host(Cs)
    eq(got, want)
    monkeypatch.setenv("ABO_GEMM_NO_SWIZZLE", "1")
    C2 = dev(Cin)
    assert gemm(Ad, Ad, C2, **kw) == GEMM_PATH_TILED
    eq(host(C2), got)
    assert np.isnan(got[:, :n][~low]).all()


# ---- split-k: partial products and their reduction ---------------------------------------------------------------------------------------
def _check_partials_and_reduce(P, A, B, rows, N, K, kmode, ks, alpha, ldc, sC, live_rows, what):
    """P: the nz partials as the kernel left them (flat, NaN-prefilled).  Chunk z ∩ range non-empty: alpha × its product on the live rows;
    empty: still NaN; rows ≥ live_rows: still NaN.  Then splitk_reduce over the same buffer = the full-range product: it read no chunk
    the GEMM skipped (NaN would show) and skipped none it wrote (integers would be missing)."""
    nz = (K + ks - 1) // ks
    Ph = host(P)
    want = np.full(Ph.shape, NAN)
    for z in range(nz):
        part = alpha * R.acc_ref(A, B, rows, N, K, kmode, chunk=(z * ks, (z + 1) * ks))
        v = want[z * sC:z * sC + rows * ldc].reshape(rows, ldc)          # a view: rows × ldc of chunk z
        v[:live_rows, :N] = part[:live_rows]
    eq(Ph, want, err_msg=what)
    ldo = N + 4
    out = dev(np.full((live_rows, ldo), NAN))
    abo._lib.check(abo._lib.lib().abo_test_splitk_reduce(0, ptr(P), ldc, sC, nz, live_rows, N, K, ks, kmode, ptr(out), ldo))
    want_o = np.full((live_rows, ldo), NAN)
    want_o[:, :N] = alpha * R.acc_ref(A, B, rows, N, K, kmode)[:live_rows]
    eq(host(out), want_o, err_msg=what + " (reduce)")


@pytest.mark.parametrize("mrows", [0, 16, 32, 48, 64])
def test_split_k_partials_and_reduce(monkeypatch, mrows):
    """mrows = 0: gemm_nt_kernel chunk by chunk; 16 … 64: gemm_skinny_kernel<1..4>, whose A has mrows rows (the rest of the 128 is NaN:
    never read) and whose partials have mrows rows (the rest stays NaN).  ksplit = 256 cuts a chunk at a tile's triangular boundary."""
    monkeypatch.delenv("ABO_GEMM_SMALL", raising=False)
    rng = np.random.default_rng(300 + mrows)
    M, N, K = 128, 384, 384
    lda, ldb, ldc = K + 6, K + 2, N + 6
    sC = M * ldc + 10
    A = R.padded(rng, M, K, lda, 64)
    B = R.padded(rng, N, K, ldb, 64)
    live = mrows if mrows else M
    A[live:, :] = NAN
    Ad, Bd = dev(A), dev(B)
    for n, (kmode, ks) in enumerate(itertools.product((K_FULL, K_B_LOWER, K_B_UPPER), (128, 256, 384))):
        alpha = R.ALPHAS[n % 4]
        nz = (K + ks - 1) // ks
        P = dev(np.full(nz * sC, NAN))
        path = gemm(Ad, Bd, P, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, sC=sC, kmode=kmode, alpha=alpha, ksplit=ks, mrows=mrows)
        assert path == (GEMM_PATH_SKINNY if mrows else GEMM_PATH_SPLITK)
        _check_partials_and_reduce(P, A, B, M, N, K, kmode, ks, alpha, ldc, sC, live, f"mrows={mrows} kmode={kmode} ksplit={ks}")


def test_split_k_of_the_tiled_kernel_with_two_tile_rows(monkeypatch):
    """M = 256: the row-tile offset of A and C inside a chunk's partial; K_A_* ranges intersected with the chunks"""
    monkeypatch.delenv("ABO_GEMM_SMALL", raising=False)
    rng = np.random.default_rng(41)
    M, N, K, ks = 256, 384, 384, 256
    lda, ldb, ldc = K + 6, K + 2, N + 6
    sC = M * ldc + 10
    A, B = R.padded(rng, M, K, lda, 64), R.padded(rng, N, K, ldb, 64)
    for kmode in range(5):
        P = dev(np.full(2 * sC, NAN))
        assert gemm(dev(A), dev(B), P, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, sC=sC, kmode=kmode, alpha=0.5, ksplit=ks,
                    mrows=32) == GEMM_PATH_SPLITK               # mrows counts for M = 128 alone
        want = np.full(2 * sC, NAN)
        for z in range(2):
            want[z * sC:z * sC + M * ldc].reshape(M, ldc)[:, :N] = 0.5 * R.acc_ref(A, B, M, N, K, kmode, chunk=(z * ks, (z + 1) * ks))
        eq(host(P), want, err_msg=f"kmode={kmode}")


# ---- qei_passd_kernel ------------------------------------------------------------------------------------------------------------------
def qei_pass(A, lda, rows16, B, ldb, nB, K, alpha, Cm, ldc, kmode=K_FULL, ksplit=0, sC=0):
    import torch
    torch.cuda.synchronize()
    return abo._lib.lib().abo_test_qei_pass(0, ptr(A), lda, rows16, ptr(B), ldb, nB, K, alpha, ptr(Cm), ldc, kmode, ksplit, sC)


@pytest.mark.parametrize("rg", [1, 2, 3, 4])
def test_qei_pass_partials_and_reduce(rg):
    """DMA-to-LDS form of the skinny product: row blocks of B are 64 wide, their triangular range that of the 128-row block tj/2"""
    rng = np.random.default_rng(500 + rg)
    rows = 16 * rg
    for n, (nB, K) in enumerate(itertools.product((128, 384), (128, 384))):
        lda, ldb, ldc = K + 6, K + 2, nB + 6
        sC = rows * ldc + 10
        A, B = R.padded(rng, rows, K, lda, 64), R.padded(rng, nB, K, ldb, 64)
        Ad, Bd = dev(A), dev(B)
        for m, (kmode, ks) in enumerate(itertools.product((K_FULL, K_B_LOWER, K_B_UPPER), (0, 128, 256))):
            alpha = R.ALPHAS[(n + m) % 4]
            kse = ks if ks else K
            nz = (K + kse - 1) // kse
            P = dev(np.full(nz * sC, NAN))
            abo._lib.check(qei_pass(Ad, lda, rows, Bd, ldb, nB, K, alpha, P, ldc, kmode, ks, sC))
            _check_partials_and_reduce(P, A, B, rows, nB, K, kmode, kse, alpha, ldc, sC, rows, f"rg={rg} nB={nB} K={K} kmode={kmode} ksplit={ks}")


def test_qei_pass_refuses_malformed_arguments_without_a_launch():
    rng = np.random.default_rng(9)
    A, B = dev(R.ints(rng, (64, 392), 64)), dev(R.ints(rng, (128, 392), 64))
    Cd = dev(np.full((64, 128), NAN))
    ok = dict(lda=392, rows16=16, ldb=392, nB=128, K=128, kmode=K_FULL, ksplit=0)
    bad = [dict(rows16=0), dict(rows16=80), dict(rows16=24), dict(nB=64), dict(K=64), dict(lda=391), dict(ldb=391), dict(kmode=K_A_LOWER),
           dict(kmode=K_A_UPPER), dict(ksplit=64)]
    for b in bad:
        a = dict(ok, **b)
        st = qei_pass(A, a["lda"], a["rows16"], B, a["ldb"], a["nB"], a["K"], 1.0, Cd, 128, a["kmode"], a["ksplit"], 0)
        assert st == ABO_EINVAL, b
        assert "refused" in abo._lib.last_error()
    assert np.isnan(host(Cd)).all()
    abo._lib.check(qei_pass(A, 392, 16, B, 392, 128, 128, 1.0, Cd, 128))
    assert not np.isnan(host(Cd)[:16]).any() and np.isnan(host(Cd)[16:]).all()


# ---- the variance contraction ------------------------------------------------------------------------------------------------------------
def var_gemm(W, ldw, Np, nvalid, Kxz, ldk, Mc, ldp, variant):
    import torch
    part = dev(np.full((Np // 128, ldp), NAN))
    torch.cuda.synchronize()
    abo._lib.check(abo._lib.lib().abo_test_var_gemm(0, ptr(W), ldw, Np, nvalid, ptr(Kxz), ldk, Mc, ptr(part), ldp, variant))
    return host(part)


def _nvalids(Np, blk):
    """Np, Np − 1, Np − 127, Np − 128, Np − 129, Np − 255 where the view still needs Np rows of `blk`-row blocks"""
    return [v for v in (Np, Np - 1, Np - 127, Np - 128, Np - 129, Np - 255) if v > 0 and v > Np - blk]


@pytest.mark.parametrize("Np", [128, 256, 384, 512, 768])
def test_variance_contraction_against_the_plain_sum_of_squares(Np):
    """partial[tb][j] = Σ_{i in block tb, i < nvalid} (W·Kxzᵀ)[i][j]² for a lower-triangular W that is dense below the diagonal (rows ≥
    nvalid included: shared storage may hold real rows there).  Np = 128, 384: var_gemm_kernel; Np = 256 (nk = 16: every stage loop of
    the zero-skipping schedule at its boundary), 512, 768: var_gemm256s_kernel (variant 0) and var_gemm_kernel (variant 1), bit for bit
    the same; nvalid in the lower and in the upper 128 rows of the last 256."""
    rng = np.random.default_rng(700 + Np)
    ldw, ldk = Np + 6, Np + 2
    W = R.tri_w(rng, Np, ldw)
    Wd = dev(W)
    two = Np % 256 == 0
    for Mc in (128, 256):
        Kxz = R.padded(rng, Mc, Np, ldk, 8, nonzero=True)
        Kd = dev(Kxz)
        ldp = Mc + 3
        for nvalid in _nvalids(Np, 256 if two else 128):
            want = np.full((Np // 128, ldp), NAN)
            want[:, :Mc] = R.var_ref(W, Kxz, Np, Mc, nvalid)
            got0 = var_gemm(Wd, ldw, Np, nvalid, Kd, ldk, Mc, ldp, 0)
            eq(got0, want, err_msg=f"Np={Np} Mc={Mc} nvalid={nvalid} variant 0")
            if two:
                got1 = var_gemm(Wd, ldw, Np, nvalid, Kd, ldk, Mc, ldp, 1)
                eq(got1, want, err_msg=f"Np={Np} Mc={Mc} nvalid={nvalid} variant 1")
                eq(got1, got0)


@pytest.mark.parametrize("Np,variant", [(384, 0), (256, 1)])
def test_the_128_row_variance_kernel_sums_its_whole_diagonal_block(Np, variant):
    """var_gemm_kernel honours k < (ti+1)·128 as a BLOCK range, as K_A_LOWER does: of a W that is dense everywhere it reads the whole
    diagonal block — non-zeros above the diagonal inside it count — and nothing to the right of it"""
    rng = np.random.default_rng(800 + Np)
    ldw, ldk, Mc = Np + 6, Np + 2, 128
    W = R.padded(rng, Np, Np, ldw, 8, nonzero=True)
    Kxz = R.padded(rng, Mc, Np, ldk, 8, nonzero=True)
    nvalid = Np - 5
    want = np.full((Np // 128, Mc + 3), NAN)
    want[:, :Mc] = R.var_ref(W, Kxz, Np, Mc, nvalid, block_range=True)
    eq(var_gemm(dev(W), ldw, Np, nvalid, dev(Kxz), ldk, Mc, Mc + 3, variant), want)
    assert not np.array_equal(want[:, :Mc], R.var_ref(np.tril(W[:, :Np]), Kxz, Np, Mc, nvalid))     # the upper triangle did count


# ---- "same bits" between kernels, on data that is NOT exact ----------------------------------------------------------------------------
def test_cross_kernel_bit_identity_on_random_data(monkeypatch):
    """The pairs csrc/gemm.hip calls "same bits" — same lane ↔ k map, same k order per accumulator: tiled vs small; skinny vs
    qei_passd; and a second run of skinny + splitk_reduce against the first (fixed-order reductions).  randn operands: every rounding
    counts, no reference and no tolerance."""
    rng = np.random.default_rng(2024)
    # tiled vs small
    M, N, K = 256, 384, 256
    A, B, C0 = dev(rng.standard_normal((M, K + 6))), dev(rng.standard_normal((N, K + 2))), rng.standard_normal((M, N))
    for kmode in range(5):
        out = {}
        for env in ("0", "1"):
            monkeypatch.setenv("ABO_GEMM_SMALL", env)
            Cd, Ctd = dev(C0), dev(np.full((N, M), NAN))
            path = gemm(A, B, Cd, Ctd, M=M, N=N, K=K, lda=K + 6, ldb=K + 2, ldc=N, ldct=M, kmode=kmode, alpha=-1.5, beta=0.5)
            assert path == (GEMM_PATH_SMALL if env == "1" else GEMM_PATH_TILED)
            out[env] = (host(Cd), host(Ctd))
        eq(out["0"][0], out["1"][0])
        eq(out["0"][1], out["1"][1])
        eq(out["0"][1], out["0"][0].T)
    monkeypatch.delenv("ABO_GEMM_SMALL")
    # skinny vs qei_passd, and skinny + reduce twice
    N, K = 384, 384
    lda, ldb, ldc = K + 6, K + 2, N + 6
    B = dev(rng.standard_normal((N, ldb)))
    for rg in (1, 2, 3, 4):
        rows = 16 * rg
        A = dev(rng.standard_normal((128, lda)))
        sC = 128 * ldc + 10
        for kmode, ks in ((K_FULL, 384), (K_FULL, 128), (K_B_LOWER, 128), (K_B_LOWER, 256)):
            nz = (K + ks - 1) // ks
            runs = []
            for _ in range(2):
                P = dev(np.full(nz * sC, NAN))
                assert gemm(A, B, P, M=128, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, sC=sC, kmode=kmode, alpha=-1.0, ksplit=ks,
                            mrows=rows) == GEMM_PATH_SKINNY
                out = dev(np.full((rows, N), NAN))
                abo._lib.check(abo._lib.lib().abo_test_splitk_reduce(0, ptr(P), ldc, sC, nz, rows, N, K, ks, kmode, ptr(out), N))
                runs.append((host(P), host(out)))
            eq(runs[0][0], runs[1][0])
            eq(runs[0][1], runs[1][1])
            assert not np.isnan(runs[0][1]).any()
            Pq = dev(np.full(nz * sC, NAN))
            abo._lib.check(qei_pass(A, lda, rows, B, ldb, N, K, -1.0, Pq, ldc, kmode, ks, sC))
            eq(host(Pq), runs[0][0], err_msg=f"rg={rg} kmode={kmode} ksplit={ks}")
