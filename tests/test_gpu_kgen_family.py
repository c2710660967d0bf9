"""Direct tests of the kernel-matrix generators (csrc/kgen_core.h, kgen_grad_core.h, kgen.hip), instantiation by instantiation (-m gpu),
through the pass-through hooks abo_test_kgen / abo_test_cand_newcol of the test build.

Method (tests/kgen_ref.py): coordinates on the grid 2⁻¹⁰·ℤ in [0, 4) and 1/ℓ a power of two make every squared distance exact, so the
device and the host hold the same r² bit for bit (tests/test_kgen_ref_cpu.py proves it for every input set used here).  Every output
buffer starts as a sentinel (NaN, the byte 0x5A, the int 77): what a kernel should not have written still is the sentinel afterwards.

What is an equality and what is a bound
  * ordinary generator: Kout == σ_f²·abo_test_kappa(r²) bit for bit (the same kappa_eval<FAM> and the same single multiply;
    test_kappa_device_math pins that hook to 60-digit mpmath); exact zeros in the padding; every residue byte == the residue of
    rint(Kout·2^sK) of the device's own Kout; res_bad; untouched sentinels.
  * μ against the long-double dot of the device's own Kout row: |Δ| ≤ (2·⌈Np/512⌉ + 10)·2⁻⁵³·(Σ_k |K_jk·α_k| + |mean|) — per sweep step two
    fma of the lane's chain, then six tree steps, three wave adds and the mean; the magnitudes are those of all the terms summed, the
    mean being one of them.  Derived, no measured slack.
  * gradient-enhanced generator against the long-double blocks: |Δ| ≤ (1.5e-15 + 2.5e-16·arg + n_op·2⁻⁵³)·σ_f²·s^q·T, T the sum of the
    magnitudes of the block's terms (kgen_ref.grad_blocks), q the number of derivatives, 1.5e-15 + 2.5e-16·arg the project's bound of the
    device's exponential and polynomial (test_kappa_device_math).  n_op, counted in kgen_grad_kernel after phi_derivs: the products
    2·il, 4·h, e_c·e_c' and il·il are exact (powers of two, grid values), which leaves ONE rounded product or fma and the multiply by σ_f²:
    n_op = 2 for K.  For d/dlog ℓ the replaced φ's are polynomials of their own (phi_derivs_dlogell: at most 6 rounded operations in
    front of the exponential's factor — √u, t, u·t, a product and two fma in the longest, the Matérn-7/2 φ' — on top of those 2): n_op = 8.
    Entries whose terms are all zero (e_c = 0, a coincident point off the diagonal of the derivative block) have T = 0: exactly ±0.

Parametrisation → instantiations launched (tick off against the switch statements of launch_kgen_dp / launch_grad_kgen_dp / launch_fam):
  test_standard_fp64[FAM]            kgen_kernel<FAM, DP, 0> for DP = 1, 2, 4, 8, 16, 32 (d = DP and DP − 1; Np = 128, 640; j0 = 0, 16);
                                     kgen_wide_kernel<FAM> at dp = 64 (d = 40) and dp = 96 (d = 70)
  test_standard_planes[FAM]          kgen_kernel<FAM, DP, 14> (full), kgen_kernel<FAM, DP, 14, true>, <FAM, DP, 8, true>, <FAM, DP, 9, true>,
                                     <FAM, DP, 10, true> (res_kmax = 128 and 384 of Np = 640), each for the six DP, Kout + planes and planes only
  test_gradient[FAM-K]               kgen_grad_kernel<FAM, DP, false, 0> for the six DP (d = DP; d = 3, 7, 13 padded), kgen_grad_wide_kernel<FAM, false> (d = 40)
  test_gradient[FAM-dlogell]         kgen_grad_kernel<FAM, DP, true, 0>, kgen_grad_wide_kernel<FAM, true>
  test_gradient[FAM-planes]          kgen_grad_kernel<FAM, DP, false, 14>
  test_cand_newcol[FAM]              cand_newcol_kernel<FAM> at dp = 1, 4, 32, 64
  test_cand_newcol_grad[FAM]         cand_newcol_grad_kernel<FAM> at dp = 1, 4, 32, 64, every training output
  test_refusals                      no kernel: what launch_kgen refuses
4 × 6 × (1 + 1 + 4) = 144 kgen_kernel, 4 wide, 3 × 6 × 3 = 54 kgen_grad_kernel, 6 grad wide."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import ABO_EINVAL, ABO_OK, AboTestKgenArgs
from oracle import gp_oracle as O

from tests import kgen_ref as R
from tests.parity_record import check

NAN = float("nan")
LD = np.longdouble
U = 2.0 ** -53
SF2 = 1.5
SENT_BYTE, SENT_INT = 0x5A, 77
eq = np.testing.assert_array_equal          # NaN == NaN at the same position


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return t.data_ptr() if t is not None else None


def kgen(*, Xs, Z, alpha=None, Kout=None, mu=None, ldk=0, M, j0=0, Mc, N, Np, d, dp, family, s, sigma_f2=SF2, mean=(0.0,), pt=1, pc=1,
         point_major=0, dlogell=0, rvalid=0, res=None, res_ld=0, res_plane=0, res_bad=None, res_n=0, res_sK=0, res_ktg=0, res_kmax=0):
    """abo_test_kgen on device tensors: the status (ABO_OK or ABO_EINVAL; anything else raises)"""
    import torch
    assert Mc % 16 == 0 and Np % 128 == 0 and Xs.numel() >= (Np if pt == 1 else N) * dp and Z.numel() >= M * d
    assert Kout is None or (ldk % 2 == 0 and ldk >= Np and Kout.numel() >= Mc * ldk)
    assert (alpha is None or alpha.numel() >= Np) and (mu is None or mu.numel() >= Mc)
    if res is not None:     # every byte a launch may write lies inside the buffers (kgen_ref.plane_offset over the chunk's rows and Np columns)
        assert res_ld % 64 == 0 and res_ld >= Np and res_plane >= R.pad_up(Mc, 256) * res_ld and res.numel() >= max(res_n, 14) * res_plane
        assert res_bad is not None and res_bad.numel() >= Mc
    mv = np.ascontiguousarray(np.asarray(mean, dtype=np.float64))
    a = AboTestKgenArgs(Xs=ptr(Xs), Z=ptr(Z), alpha=ptr(alpha), Kout=ptr(Kout), mu=ptr(mu), ldk=ldk, M=M, j0=j0, Mc=Mc, N=N, Np=Np, d=d, dp=dp,
                        family=family, s=s, sigma_f2=sigma_f2, mean_vec=mv.ctypes.data, pt=pt, pc=pc, point_major=point_major, dlogell=dlogell,
                        rvalid=rvalid, n_mean=mv.size, res=ptr(res), res_ld=res_ld, res_plane=res_plane, res_bad=ptr(res_bad), res_n=res_n,
                        res_sK=res_sK, res_ktg=res_ktg, res_kmax=res_kmax)
    torch.cuda.synchronize()
    st = abo._lib.lib().abo_test_kgen(0, C.byref(a))
    if st not in (ABO_OK, ABO_EINVAL):
        abo._lib.check(st)
    return st


def kappa_dev(family, r2):
    """abo_test_kappa: kappa_eval<FAM> with the device math, at the exact r²"""
    import torch
    x = dev(np.asarray(r2, dtype=np.float64).reshape(-1))
    out = torch.empty_like(x)
    torch.cuda.synchronize()
    abo._lib.check(abo._lib.lib().abo_test_kappa(0, family, x.data_ptr(), out.data_ptr(), x.numel()))
    return host(out).reshape(np.shape(r2))


def scaled(X, s, rows, dp):
    Xs = np.zeros((rows, dp))
    Xs[:X.shape[0], :X.shape[1]] = X * s
    return Xs


def padded_alpha(rng, n, Np):
    a = np.zeros(Np)
    a[:n] = rng.standard_normal(n) * 2.0 ** rng.integers(-20, 3, n)      # small and large weights side by side
    return a


def mu_ratio(mu, K, alpha, mean, Np):
    """achieved |Δμ| over the derived bound, against the long-double dot of the device's own rows (K [rows][cols], alpha [cols])"""
    prod = K.astype(LD) * alpha.astype(LD)[None, :]
    ref = np.asarray(mean, dtype=LD) + prod.sum(1)
    mag = np.abs(prod).sum(1) + np.abs(np.asarray(mean, dtype=LD))
    bound = (2 * -(-Np // 512) + 10) * U * mag
    err = np.abs(mu.astype(LD) - ref)
    assert np.all(err[bound == 0] == 0)
    nz = bound > 0
    return float(np.max(err[nz] / bound[nz])) if np.any(nz) else 0.0


# ---- (a), (b): the ordinary generator ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _std_case(family, d, Np):
    """inputs and the bit-exact expectation σ_f²·κ(r²) [M][N], computed once and shared"""
    X, Z, s = R.standard_inputs(d, Np)
    want = SF2 * kappa_dev(family, R.r2_matrix(X, Z, s))
    for a in (X, Z, want):
        a.setflags(write=False)
    return X, Z, s, want


def _expected_K(want, M, Mc, j0, N, Np, ldk, kend):
    """the whole Kout buffer after a launch over the columns k < kend: values, exact zeros, NaN where nothing is written"""
    full = np.full((Mc, ldk), NAN)
    full[:, :kend] = 0.0
    rows = min(Mc, max(M - j0, 0))
    full[:rows, :min(N, kend)] = want[j0:j0 + rows, :min(N, kend)]
    return full


def _no_negative_zero(K, kend):
    assert not np.any(np.signbit(K[:, :kend]) & (K[:, :kend] == 0))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_standard_fp64(family):
    import torch
    M, Mc, mean = R.M_STD, 48, 0.375
    worst = 0.0
    for dp, d in R.STD_DIMS:
        for Np, j0 in ((128, 0), (640, 0)) + (((128, 16),) if d == dp or dp > 32 else ()):
            X, Z, s, want = _std_case(family, d, Np)
            N, ldk = Np - 3, Np + 6
            rng = np.random.default_rng(Np + d)
            alpha = padded_alpha(rng, N, Np)
            Xs_d, Z_d, a_d = dev(scaled(X, s, Np, dp)), dev(Z), dev(alpha)
            K_d, mu_d = dev(np.full((Mc, ldk), NAN)), dev(np.full(Mc, NAN))
            common = dict(Xs=Xs_d, Z=Z_d, M=M, j0=j0, Mc=Mc, N=N, Np=Np, d=d, dp=dp, family=family, s=s, mean=(mean,))
            what = f"family={family} dp={dp} d={d} Np={Np} j0={j0}"
            assert kgen(alpha=a_d, Kout=K_d, mu=mu_d, ldk=ldk, **common) == ABO_OK, what
            K, mu = host(K_d), host(mu_d)
            eq(K, _expected_K(want, M, Mc, j0, N, Np, ldk, Np), err_msg=what)          # bit for bit; zeros; NaN behind Np
            _no_negative_zero(K, Np)
            worst = max(worst, mu_ratio(mu, K[:, :Np], alpha, mean, Np))
            # no alpha: μ is the mean, exactly; no Kout, no μ: nothing is written
            K2_d, mu2_d = dev(np.full((Mc, ldk), NAN)), dev(np.full(Mc, NAN))
            assert kgen(mu=mu2_d, **common) == ABO_OK
            eq(host(mu2_d), np.full(Mc, mean), err_msg=what)
            assert kgen(alpha=a_d, **common) == ABO_OK
            assert bool(torch.isnan(K2_d).all()) and bool((mu2_d == mean).all()), what
    check(f"kgen_family_std_fam{family}", "mu_over_bound", worst, 1.0, tighten=False)


def _plane_case(family, dp, d, Np, n, kmax, *, j0=0, nan_row=None, bufs):
    """one launch with Kout + planes and one with planes only; returns the achieved μ ratio"""
    import torch
    M, Mc, mean = R.M_STD, 48, -0.25
    X, Z, s, want = _std_case(family, d, Np)
    N, ldk, kend = Np - 3, Np + 6, (kmax or Np)
    res_ld = R.pad_up(Np, 256)
    res_plane = 256 * res_ld
    sK = R.k_scale(SF2)
    rng = np.random.default_rng(7 * Np + d + n)
    alpha = padded_alpha(rng, N, Np)
    if nan_row is not None:
        Z = Z.copy()
        Z[nan_row, d - 1] = NAN
    Xs_d, Z_d, a_d = dev(scaled(X, s, Np, dp)), dev(Z), dev(alpha)
    K_d, mu_d = dev(np.full((Mc, ldk), NAN)), dev(np.full(Mc, NAN))
    res_d, res2_d, bad_d = bufs
    res_d.fill_(SENT_BYTE), res2_d.fill_(SENT_BYTE), bad_d.fill_(SENT_INT)
    common = dict(Xs=Xs_d, Z=Z_d, alpha=a_d, M=M, j0=j0, Mc=Mc, N=N, Np=Np, d=d, dp=dp, family=family, s=s, mean=(mean,), res_ld=res_ld,
                  res_plane=res_plane, res_bad=bad_d, res_n=n, res_sK=sK, res_kmax=kmax)
    what = f"family={family} dp={dp} d={d} Np={Np} n={n} kmax={kmax} j0={j0} nan_row={nan_row}"
    assert kgen(Kout=K_d, mu=mu_d, ldk=ldk, res=res_d, **common) == ABO_OK, what
    K, mu, bad = host(K_d), host(mu_d), host(bad_d)
    planes = host(res_d[:(n + 1) * res_plane]).reshape(n + 1, res_plane)
    # Kout: the same bits as the fp64 build over the columns of the launch, nothing behind them
    exp_K = _expected_K(want, M, Mc, j0, N, Np, ldk, kend)
    ok_rows = np.ones(Mc, dtype=bool)
    if nan_row is not None:
        exp_K[nan_row - j0, :kend] = NAN
        ok_rows[nan_row - j0] = False
    eq(K, exp_K, err_msg=what)
    eq(bad[:Mc], (~ok_rows).astype(np.int32), err_msg=what)                      # padding rows included: every entry is written
    # planes: every byte of the chunk's rows and the launch's columns is the residue of the device's own value; the rest is untouched
    jj, kk = np.meshgrid(np.arange(Mc), np.arange(kend), indexing="ij")
    off = R.plane_offset(jj, kk, res_ld)
    assert off.max() < res_plane
    x = np.rint(np.where(ok_rows[:, None], K[:, :kend], 0.0) * 2.0 ** sK)
    assert np.max(np.abs(x)) < 2.0 ** 52
    exp_b = R.residues(x, n)
    got_b = planes[:n][:, off]
    eq(got_b[:, ok_rows], exp_b[:, ok_rows], err_msg=what)
    untouched = np.ones(res_plane, dtype=bool)
    untouched[off.reshape(-1)] = False
    assert np.all(planes[:n][:, untouched] == SENT_BYTE) and np.all(planes[n] == SENT_BYTE), what
    ratio = mu_ratio(mu[ok_rows], K[ok_rows, :kend], alpha[:kend], mean, Np)
    # planes only: the same bytes, the same μ, the same res_bad
    mu2_d = dev(np.full(Mc, NAN))
    bad_d.fill_(SENT_INT)
    assert kgen(mu=mu2_d, res=res2_d, **common) == ABO_OK, what
    assert torch.equal(res2_d[:(n + 1) * res_plane], res_d[:(n + 1) * res_plane]), what
    eq(host(mu2_d), mu, err_msg=what)
    eq(host(bad_d), bad, err_msg=what)
    return ratio


@pytest.mark.parametrize("family", R.FAMILIES)
def test_standard_planes(family):
    import torch
    plane_max = 256 * R.pad_up(640, 256)
    bufs = (torch.empty(15 * plane_max, dtype=torch.int8, device="cuda"), torch.empty(15 * plane_max, dtype=torch.int8, device="cuda"),
            torch.empty(48, dtype=torch.int32, device="cuda"))
    worst = 0.0
    for dp, d in R.STD_DIMS:
        if dp > 32:
            continue
        cases = [(640, 14, 0), (640, 8, 128)]
        if d == dp:
            cases += [(128, 14, 0)] + [(640, n, kmax) for n in (14, 8, 9, 10) for kmax in (128, 384) if (n, kmax) != (8, 128)]
        for Np, n, kmax in cases:
            worst = max(worst, _plane_case(family, dp, d, Np, n, kmax, bufs=bufs))
        if d == dp:
            # a chunk offset, and a candidate with a NaN coordinate (full and partial launch)
            worst = max(worst, _plane_case(family, dp, d, 128, 14, 0, j0=16, bufs=bufs))
            worst = max(worst, _plane_case(family, dp, d, 128, 14, 0, nan_row=5, bufs=bufs))
            worst = max(worst, _plane_case(family, dp, d, 640, 9, 384, nan_row=33, bufs=bufs))
    check(f"kgen_family_planes_fam{family}", "mu_over_bound", worst, 1.0, tighten=False)


# ---- (c): the gradient-enhanced generator -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _grad_ref(family, d, Np, M, pc, dlogell):
    """long-double blocks and their bounds for the candidate outputs q < pc, computed once and shared by the builds"""
    X, Z, s = R.grad_inputs(d, Np, M)
    V, T, ND = R.grad_blocks(family, X, Z, s, SF2, dlogell=bool(dlogell))
    V, T, ND = V[:, :pc].copy(), T[:, :pc].copy(), ND[:pc]
    u = R.r2_matrix(X, Z, s)
    n_op = 8 if dlogell else 2                                                   # counted in the module text
    tol = ((R.kappa_rel_bound(family, u) + n_op * U).astype(LD)[:, None, :, None] * LD(SF2)
           * np.power(LD(s), ND.astype(LD))[None, :, None, :] * T)
    for a in (X, Z, V, tol):
        a.setflags(write=False)
    return X, Z, s, V, tol, ND


GRAD_BUILDS = ("K", "dlogell", "planes")


@pytest.mark.parametrize("build", GRAD_BUILDS)
@pytest.mark.parametrize("family", R.GRAD_FAMILIES)
def test_gradient(family, build):
    import torch
    dlogell = int(build == "dlogell")
    ktg, sK = 3, R.k_scale(2.0 * SF2)
    worst_k = worst_mu = 0.0
    if build == "planes":
        plane_max = 256 * R.pad_up(640, 256)
        res_d = torch.empty(15 * plane_max, dtype=torch.int8, device="cuda")
    for dp, d in R.GRAD_DIMS:
        if build == "planes" and dp > 32:
            continue
        pt = d + 1
        # (Np, M, pc, point_major, chunk offset, partly appended point)
        cases = [(640, 37, 1, 0, 16, 0), (640, 7, pt, 0, 16 if 7 * pt > 32 else 0, 0), (640, 7, pt, 1, 0, 1)]
        if d == dp:
            cases.append((128, 7, pt, 1, 0, 0))
        for Np, M, pc, pm, j0, partly in cases:
            X, Z, s, V, tol, ND = _grad_ref(family, d, Np, M, pc, dlogell)
            N = X.shape[0]
            R_cols = N * pt - 2 if partly else N * pt
            rows_total = M * pc
            rows = rows_total - j0
            Mc, ldk = R.pad_up(rows, 16), Np + 4
            want, wtol = R.as_rows(V, pc, pm)[j0:], R.as_rows(tol, pc, pm)[j0:]
            jrow, qrow = (a[j0:] for a in R.row_index(M, pc, pm))
            rng = np.random.default_rng(d + Np + M + pc)
            alpha = padded_alpha(rng, R_cols, Np)
            mean = np.round(rng.uniform(-1, 1, pt), 3)
            K_d, mu_d = dev(np.full((Mc, ldk), NAN)), dev(np.full(Mc, NAN))
            args = dict(Xs=dev(scaled(X, s, Np, dp)), Z=dev(Z), alpha=dev(alpha), Kout=K_d, mu=mu_d, ldk=ldk, M=M, j0=j0, Mc=Mc, N=N, Np=Np, d=d,
                        dp=dp, family=family, s=s, mean=mean, pt=pt, pc=pc, point_major=pm, dlogell=dlogell, rvalid=R_cols if partly else 0)
            if build == "planes":
                res_ld = R.pad_up(Np, 256)
                res_plane = R.pad_up(Mc, 256) * res_ld
                bad_d = dev(np.full(Mc, SENT_INT, dtype=np.int32))
                res_d.fill_(SENT_BYTE)
                args.update(res=res_d, res_ld=res_ld, res_plane=res_plane, res_bad=bad_d, res_n=14, res_sK=sK, res_ktg=ktg)
            what = f"family={family} build={build} dp={dp} d={d} Np={Np} M={M} pc={pc} point_major={pm} j0={j0} rvalid={args['rvalid']}"
            assert kgen(**args) == ABO_OK, what
            K, mu = host(K_d), host(mu_d)
            # the frame: exact zeros right of the valid training rows and below the last candidate row, NaN behind Np
            assert np.all(np.isnan(K[:, Np:])) and np.all(np.isfinite(K[:, :Np])), what
            assert np.all(K[:rows, R_cols:Np] == 0) and np.all(K[rows:, :Np] == 0), what
            got = K[:rows, :R_cols]
            err = np.abs(got.astype(LD) - want[:, :R_cols])
            lim = wtol[:, :R_cols]
            zero = lim == 0
            assert np.all(got[zero] == 0), what                                  # e_c = 0, coincident points: exactly ±0
            assert np.any(zero) or d == 1
            assert np.all(err <= lim), (what, float(np.max(err[~zero] / lim[~zero])))
            worst_k = max(worst_k, float(np.max(err[~zero] / lim[~zero])))
            eq(mu[rows:], np.zeros(Mc - rows), err_msg=what)
            worst_mu = max(worst_mu, mu_ratio(mu[:rows], K[:rows, :Np], alpha, mean[qrow], Np))
            if build == "planes":
                eq(host(bad_d), np.zeros(Mc, dtype=np.int32), err_msg=what)
                planes = host(res_d[:15 * res_plane]).reshape(15, res_plane)
                jj, kk = np.meshgrid(np.arange(Mc), np.arange(Np), indexing="ij")
                off = R.plane_offset(jj, kk, res_ld)
                assert off.max() < res_plane
                nd = np.zeros((Mc, Np), dtype=np.int64)
                nd[:rows] = (qrow > 0)[:, None].astype(np.int64) + ((np.arange(Np) % pt) > 0)[None, :]
                x = np.rint(K[:, :Np] * 2.0 ** (sK - ktg * nd).astype(np.float64))
                assert np.max(np.abs(x)) < 2.0 ** 52
                eq(planes[:14][:, off], R.residues(x, 14), err_msg=what)
                untouched = np.ones(res_plane, dtype=bool)
                untouched[off.reshape(-1)] = False
                assert np.all(planes[:14][:, untouched] == SENT_BYTE) and np.all(planes[14] == SENT_BYTE), what
        if build == "planes" and d == dp:
            # a candidate with a NaN coordinate: every output row of it is NaN against every valid training row and flagged, no other row is
            X, Z, s, _, _, _ = _grad_ref(family, d, 128, 7, pt, 0)
            N, Np, rows = X.shape[0], 128, 7 * pt
            Mc, ldk = R.pad_up(rows, 16), Np + 4
            Zn = Z.copy()
            Zn[2, d - 1] = NAN
            K_d, bad_d = dev(np.full((Mc, ldk), NAN)), dev(np.full(Mc, SENT_INT, dtype=np.int32))
            assert kgen(Xs=dev(scaled(X, s, Np, dp)), Z=dev(Zn), Kout=K_d, ldk=ldk, M=7, Mc=Mc, N=N, Np=Np, d=d, dp=dp, family=family, s=s,
                        mean=np.zeros(pt), pt=pt, pc=pt, point_major=1, res=res_d, res_ld=256, res_plane=R.pad_up(Mc, 256) * 256, res_bad=bad_d,
                        res_n=14, res_sK=sK, res_ktg=ktg) == ABO_OK
            K, isn = host(K_d), np.zeros(Mc, dtype=bool)
            isn[2 * pt:3 * pt] = True
            assert np.all(np.isnan(K[isn, :N * pt])) and np.all(np.isfinite(K[~isn, :Np])), (family, dp)
            eq(host(bad_d), isn.astype(np.int32), err_msg=f"family={family} dp={dp} NaN candidate")
    check(f"kgen_family_grad_fam{family}_{build}", "k_over_bound", worst_k, 1.0, tighten=False)
    check(f"kgen_family_grad_fam{family}_{build}", "mu_over_bound", worst_mu, 1.0, tighten=False)


# ---- (d): one column of the same matrices -----------------------------------------------------------------------------------------------
NEWCOL_DIMS = ((1, 1), (4, 4), (32, 32), (64, 40))


def newcol(Xs, Z, Kzx, ld, M, col, d, dp, family, s, grad=0, pt=0, q=0):
    import torch
    torch.cuda.synchronize()
    st = abo._lib.lib().abo_test_cand_newcol(0, ptr(Xs), ptr(Z), ptr(Kzx), ld, M, col, grad, pt, q, d, dp, family, s, SF2)
    if st not in (ABO_OK, ABO_EINVAL):
        abo._lib.check(st)
    return st


@pytest.mark.parametrize("family", R.FAMILIES)
def test_cand_newcol(family):
    M = 261                                                                     # two workgroups, the second partly filled
    for dp, d in NEWCOL_DIMS:
        X, Z, s = R.standard_inputs(d, 128, M=M)
        N, ld = X.shape[0], X.shape[0] + 3
        want = SF2 * kappa_dev(family, R.r2_matrix(X, Z, s))
        Xs_d, Z_d = dev(scaled(X, s, 128, dp)), dev(Z)
        for col in (0, N - 1):
            K_d = dev(np.full((M + 2, ld), NAN))
            assert newcol(Xs_d, Z_d, K_d, ld, M, col, d, dp, family, s) == ABO_OK
            exp = np.full((M + 2, ld), NAN)
            exp[:M, col] = want[:, col]
            eq(host(K_d), exp, err_msg=f"family={family} dp={dp} col={col}")     # the column bit for bit, no other element touched


@pytest.mark.parametrize("family", R.GRAD_FAMILIES)
def test_cand_newcol_grad(family):
    M = 261
    worst = 0.0
    for dp, d in NEWCOL_DIMS:
        X, Z, s = R.standard_inputs(d, 128, M=M)
        N, pt = X.shape[0], d + 1
        pts = (0, N - 1)
        V, T, ND = R.grad_blocks(family, X[list(pts)], Z, s, SF2)
        u = R.r2_matrix(X[list(pts)], Z, s)
        tol = (R.kappa_rel_bound(family, u) + 2 * U).astype(LD)[:, :, None] * LD(SF2) * np.power(LD(s), ND[0].astype(LD))[None, None, :] * T[:, 0]
        ld = 2 * pt + 1
        K_d = dev(np.full((M + 2, ld), NAN))
        Xs_d, Z_d = dev(scaled(X, s, 128, dp)), dev(Z)
        for n, i in enumerate(pts):
            for q in range(pt):
                assert newcol(Xs_d, Z_d, K_d, ld, M, n * pt + q, d, dp, family, s, grad=1, pt=i, q=q) == ABO_OK
        K = host(K_d)
        assert np.all(np.isnan(K[M:])) and np.all(np.isnan(K[:, 2 * pt])) and np.all(np.isfinite(K[:M, :2 * pt]))
        got = K[:M, :2 * pt].reshape(M, 2, pt)
        err, zero = np.abs(got.astype(LD) - V[:, 0]), tol == 0
        assert np.all(got[zero] == 0) and np.any(zero)
        assert np.all(err <= tol), (family, dp, float(np.max(err[~zero] / tol[~zero])))
        worst = max(worst, float(np.max(err[~zero] / tol[~zero])))
    check(f"kgen_family_newcol_grad_fam{family}", "k_over_bound", worst, 1.0, tighten=False)


# ---- (e): what the launcher refuses ---------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    M, Mc, Np, d = R.M_STD, 48, 640, 4
    X, Z, s = R.standard_inputs(d, Np)
    N, ldk = Np - 3, Np + 6
    res_ld = R.pad_up(Np + 128, 256)
    res_plane = 256 * res_ld
    K_d, mu_d = dev(np.full((Mc, ldk), NAN)), dev(np.full(Mc, NAN))
    res_d = torch.full((14 * res_plane,), SENT_BYTE, dtype=torch.int8, device="cuda")
    bad_d = dev(np.full(Mc, SENT_INT, dtype=np.int32))
    a_d, Z_d = dev(np.ones(Np)), dev(Z)

    def refused(dp, what, **kw):
        planes = kw.pop("planes", None)
        args = dict(Xs=dev(np.ones((Np, max(dp, d)))), Z=Z_d, alpha=a_d, Kout=K_d, mu=mu_d, ldk=ldk, M=M, Mc=Mc, N=N, Np=Np, d=d, dp=dp, family=O.SE, s=s)
        if planes is not None:
            args.update(res=res_d, res_ld=res_ld, res_plane=res_plane, res_bad=bad_d, res_n=planes, res_sK=R.k_scale(SF2))
        args.update(kw)
        assert kgen(**args) == ABO_EINVAL, what
        assert "refused" in abo._lib.last_error(), what
        torch.cuda.synchronize()
        assert bool(torch.isnan(K_d).all()) and bool(torch.isnan(mu_d).all()), what
        assert bool((res_d == SENT_BYTE).all()) and bool((bad_d == SENT_INT).all()), what

    refused(3, "a dp outside the dispatch table")
    refused(48, "a wide dp that is no multiple of 32")
    refused(12, "a dp outside the table with planes", planes=14)
    refused(5, "a gradient dp outside the table", pt=d + 1, pc=1, N=100, mean=np.zeros(d + 1))
    refused(4, "res_kmax no multiple of 128", planes=14, res_kmax=192)
    refused(4, "res_kmax beyond Np", planes=14, res_kmax=Np + 128)
    refused(4, "res_kmax beyond Np on a short plan", planes=8, res_kmax=Np + 128)
    for n in (8, 9, 10):
        refused(4, "a short plan without res_kmax", planes=n)
    refused(4, "a moduli count without fused planes", planes=12, res_kmax=128)
    refused(64, "planes with dp > 32", planes=14)
    refused(64, "planes with dp > 32, partial", planes=8, res_kmax=128)
    refused(4, "an unknown family", family=7)
    refused(4, "Matérn-3/2 with gradients", family=O.MATERN32, pt=d + 1, pc=1, N=100, mean=np.zeros(d + 1))
    refused(4, "gradient planes with d/dlog ℓ", planes=14, dlogell=1, pt=d + 1, pc=1, N=100, mean=np.zeros(d + 1))
