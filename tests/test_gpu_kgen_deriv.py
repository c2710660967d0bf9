"""Direct tests of the value-only model's derivative cross-kernel generator (csrc/kgen_deriv.hip), through the pass-through hook
abo_test_kgen_deriv of the test build (-m gpu).

Method, as in tests/test_gpu_kgen_family.py (tests/kgen_ref.py): coordinates on the grid 2⁻¹⁰·ℤ in [0, 4) and 1/ℓ a power of two make every
scaled difference e_c and every squared distance u exact on the device and on the host.  Buffers start as NaN: what the kernel should
not have written still is NaN afterwards.

Bounds (derived, no measured slack)
  * Kout against the long-double blocks V[j][q][k][0] of kgen_ref.grad_blocks (the rows of a value training point):
    |Δ| ≤ (kappa_rel_bound(u) + n_op·2⁻⁵³)·σ_f²·s^[q>0]·T, kappa_rel_bound = the project's bound of the device's exponential and polynomial,
    T the magnitude of the block's one term (|φ|, or 2|φ'||e_c|).  n_op, counted in kgen_deriv_kernel behind phi_derivs: a value row is
    ONE rounded product (σ_f²·φ); a derivative row is TWO — cg·φ' and its product with e_c, cg = −2·s·σ_f² being exact for a power-of-two s
    and σ_f² = 1.5.  e_c = 0 (a coincident point, or a shared coordinate) gives T = 0: exactly ±0.
  * mu_rows against the long-double dot of the device's own row with alpha: |Δ| ≤ N·2⁻⁵³·(Σ_k |K_rk·α_k| + |mean|) — every one of the at most
    N + 10 additions of the fixed-order sum (the lane's chain, six tree steps, three wave adds, the mean) rounds a partial sum no larger
    than the sum of the magnitudes, and its fma rounds once per term; N ≥ 128 > ⌈N/256⌉ + 10 steps of any one chain."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import ABO_EINVAL, ABO_OK
from oracle import gp_oracle as O

from tests import kgen_ref as R
from tests.parity_record import check

NAN = float("nan")
LD = np.longdouble
U = 2.0 ** -53
SF2, MEAN = 1.5, 0.375
FAMILIES = (O.SE, O.MATERN52, O.MATERN72)
#         N,  Np,  d, dp,  M, pt0
SHAPES = [(200, 256, 1, 1, 5, 2), (200, 256, 3, 4, 5, 2), (200, 256, 32, 32, 5, 2),
          (128, 128, 1, 1, 5, 2), (128, 128, 3, 4, 5, 2), (128, 128, 32, 32, 5, 2),
          (600, 640, 3, 4, 11, 1),          # three sweep steps; three workgroups of four points, the last one with two
          (200, 256, 13, 16, 6, 1)]         # dp = 16: two points per workgroup, the last one with one


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def kgen_deriv(Xs, alpha, Z, K, mu, *, ldk, M, pt0, npts, rows_pad, N, Np, d, dp, family, s):
    import torch
    assert Xs.numel() >= Np * dp and Z.numel() >= M * d and K.numel() >= rows_pad * ldk and (mu is None or mu.numel() >= rows_pad)
    assert alpha is None or alpha.numel() >= Np
    torch.cuda.synchronize()
    st = abo._lib.lib().abo_test_kgen_deriv(0, Xs.data_ptr(), alpha.data_ptr() if alpha is not None else None, Z.data_ptr(), K.data_ptr(),
                                            mu.data_ptr() if mu is not None else None, ldk, M, pt0, npts, rows_pad, N, Np, d, dp, family,
                                            s, SF2, MEAN)
    if st not in (ABO_OK, ABO_EINVAL):
        abo._lib.check(st)
    return st


@functools.lru_cache(maxsize=None)
def inputs(N, d, M):
    rng = np.random.default_rng(300000 + 1000 * d + N + 7 * M)
    X = R.grid_points(rng, N, d)
    Z = R.grid_points(rng, M, d)
    Z[M - 1] = X[N - 1]                                                          # a query point equal to a training point
    Z[M - 2] = X[min(7, N - 1)]
    Z[M - 2, 0] = (Z[M - 2, 0] + 0.5) % 4.0                                      # … and one that shares every coordinate but the first
    R.assert_exact_r2(X, Z, R.s_of(d))
    for a in (X, Z):
        a.setflags(write=False)
    return X, Z, R.s_of(d)


@functools.lru_cache(maxsize=None)
def reference(family, N, d, M, pt0):
    """long-double rows [npts·p][N] of the chunk and their bounds, computed once"""
    X, Z, s = inputs(N, d, M)
    Zc = Z[pt0:]
    V, T, ND = R.grad_blocks(family, X, Zc, s, SF2)
    u = R.r2_matrix(X, Zc, s)
    p = d + 1
    n_op = np.where(np.arange(p) == 0, 1, 2).astype(LD)
    tol = ((R.kappa_rel_bound(family, u).astype(LD)[:, None, :] + n_op[None, :, None] * LD(U)) * LD(SF2)
           * np.power(LD(s), ND[:, 0].astype(LD))[None, :, None] * T[:, :, :, 0])
    want = V[:, :, :, 0].reshape(Zc.shape[0] * p, N)
    return want, tol.reshape(Zc.shape[0] * p, N)


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_padding_and_means(family):
    worst_k = worst_mu = 0.0
    for N, Np, d, dp, M, pt0 in SHAPES:
        X, Z, s = inputs(N, d, M)
        p, npts = d + 1, M - pt0
        rows, rows_pad, ldk = npts * p, R.pad_up(npts * p, 128), Np + 4
        want, tol = reference(family, N, d, M, pt0)
        rng = np.random.default_rng(N + d)
        alpha = np.zeros(Np)
        alpha[:N] = rng.standard_normal(N) * 2.0 ** rng.integers(-20, 3, N)
        alpha_dev = alpha.copy()
        alpha_dev[N:] = NAN                                                     # only k < N may be read
        Xs = np.zeros((Np, dp))
        Xs[:N, :d] = X * s
        K_d, mu_d = dev(np.full((rows_pad + 2, ldk), NAN)), dev(np.full(rows_pad + 3, NAN))
        what = f"family={family} N={N} Np={Np} d={d} dp={dp} M={M} pt0={pt0}"
        args = dict(ldk=ldk, M=M, pt0=pt0, npts=npts, rows_pad=rows_pad, N=N, Np=Np, d=d, dp=dp, family=family, s=s)
        assert kgen_deriv(dev(Xs), dev(alpha_dev), dev(Z), K_d, mu_d, **args) == ABO_OK, what
        K, mu = K_d.cpu().numpy(), mu_d.cpu().numpy()
        # the frame: NaN behind Np and behind rows_pad, exact zeros in the padding columns and rows
        assert np.all(np.isnan(K[:, Np:])) and np.all(np.isnan(K[rows_pad:])) and np.all(np.isnan(mu[rows_pad:])), what
        assert np.all(np.isfinite(K[:rows_pad, :Np])) and np.all(K[:rows_pad, N:Np] == 0) and np.all(K[rows:rows_pad, :Np] == 0), what
        assert np.all(mu[rows:rows_pad] == 0), what
        got = K[:rows, :N]
        err = np.abs(got.astype(LD) - want)
        zero = tol == 0
        assert np.all(got[zero] == 0) and np.any(zero), what                  # e_c = 0: exactly ±0
        print(f"{what}: max |dK| / bound = {float(np.max(err[~zero] / tol[~zero])):.3f}")
        assert np.all(err <= tol), (what, float(np.max(err[~zero] / tol[~zero])))
        worst_k = max(worst_k, float(np.max(err[~zero] / tol[~zero])))
        # the means, against the device's own rows
        mean = np.tile(np.concatenate([[MEAN], np.zeros(d)]), npts)
        prod = K[:rows, :N].astype(LD) * alpha[:N].astype(LD)[None, :]
        ref = mean.astype(LD) + prod.sum(1)
        bound = N * U * (np.abs(prod).sum(1) + np.abs(mean))
        merr = np.abs(mu[:rows].astype(LD) - ref)
        assert np.all(merr[bound == 0] == 0), what
        nz = bound > 0
        print(f"{what}: max |dmu| / bound = {float(np.max(merr[nz] / bound[nz])):.3e}")
        assert np.all(merr <= bound), what
        worst_mu = max(worst_mu, float(np.max(merr[nz] / bound[nz])))
        # the same bits on a second launch; no alpha: the means are the prior means; no mu_rows: Kout alone
        K2_d, mu2_d = dev(np.full((rows_pad + 2, ldk), NAN)), dev(np.full(rows_pad + 3, NAN))
        assert kgen_deriv(dev(Xs), dev(alpha_dev), dev(Z), K2_d, mu2_d, **args) == ABO_OK
        assert K2_d.cpu().numpy().tobytes() == K.tobytes() and mu2_d.cpu().numpy().tobytes() == mu.tobytes(), what
        mu3_d = dev(np.full(rows_pad + 3, NAN))
        assert kgen_deriv(dev(Xs), None, dev(Z), K2_d, mu3_d, **args) == ABO_OK
        np.testing.assert_array_equal(mu3_d.cpu().numpy()[:rows], mean, err_msg=what)
        K4_d = dev(np.full((rows_pad + 2, ldk), NAN))
        assert kgen_deriv(dev(Xs), dev(alpha_dev), dev(Z), K4_d, None, **args) == ABO_OK
        assert K4_d.cpu().numpy().tobytes() == K.tobytes(), what
    check(f"kgen_deriv_fam{family}", "k_over_bound", worst_k, 1.0, tighten=False)
    check(f"kgen_deriv_fam{family}", "mu_over_bound", worst_mu, 1.0, tighten=False)


def test_refusals():
    import torch
    N, Np, d, M = 200, 256, 3, 5
    X, Z, s = inputs(N, d, M)
    rows_pad, ldk = 128, Np + 4
    K_d, mu_d = dev(np.full((rows_pad, ldk), NAN)), dev(np.full(rows_pad, NAN))
    Xs_d, a_d = dev(np.ones((Np, 64))), dev(np.ones(Np))
    Z33 = dev(np.ones((M, 33)))

    def refused(what, Zd=None, **kw):
        args = dict(ldk=ldk, M=M, pt0=2, npts=3, rows_pad=rows_pad, N=N, Np=Np, d=d, dp=4, family=O.SE, s=s)
        args.update(kw)
        st = abo._lib.lib().abo_test_kgen_deriv(0, Xs_d.data_ptr(), a_d.data_ptr(), (Zd if Zd is not None else dev(Z)).data_ptr(), K_d.data_ptr(),
                                                mu_d.data_ptr(), args["ldk"], args["M"], args["pt0"], args["npts"], args["rows_pad"], args["N"],
                                                args["Np"], args["d"], args["dp"], args["family"], args["s"], SF2, MEAN)
        assert st == ABO_EINVAL, what
        assert "abo_test_kgen_deriv" in abo._lib.last_error() and "refused" in abo._lib.last_error(), what
        torch.cuda.synchronize()
        assert bool(torch.isnan(K_d).all()) and bool(torch.isnan(mu_d).all()), what

    refused("d = 33", Zd=Z33, d=33, dp=64, rows_pad=128, npts=3)
    refused("Matérn-3/2", family=O.MATERN32)
    refused("an unknown family", family=7)
    refused("a dp outside the table", dp=3)
    refused("dp below d", dp=2)
    refused("Np no multiple of 128", Np=200)
    refused("N beyond Np", N=Np + 1)
    refused("ldk below Np", ldk=Np - 2)
    refused("a chunk beyond M", pt0=3, npts=3)
    refused("rows_pad below the chunk's rows", rows_pad=11)
