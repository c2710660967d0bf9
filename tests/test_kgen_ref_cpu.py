"""CPU tests of tests/kgen_ref.py — the reference tests/test_gpu_kgen_family.py holds the kernel-matrix generators to: its long-double
kernels against the fp64 oracles, its d/dlog ℓ blocks against a central difference of its own blocks, the plane layout, and the proof
that every input set of the GPU tests has an exact r²."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from oracle import grad_oracle as GO
from tests import kgen_ref as R


def test_long_double_is_wide_enough_or_mpmath_stands_in():
    assert R.HAVE_LD == bool(np.finfo(np.longdouble).eps < 2e-19)
    if not R.HAVE_LD:
        import mpmath
        assert mpmath.mp.dps >= 40


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("ell", [1.0, 0.5, 2.0])
def test_kernel_ref_against_the_oracle(family, ell):
    rng = np.random.default_rng(family)
    for d in (1, 3, 8, 40):
        X, Z = R.grid_points(rng, 33, d), R.grid_points(rng, 9, d)
        Z[0] = X[0]
        sf2 = 1.5
        ref = R.kernel_ref(family, R.r2_matrix(X, Z, 1.0 / ell), sf2)                  # [j][i]
        orc = O.kernel_matrix(family, ell, sf2, X, Z).T
        assert np.max(np.abs(ref - orc)) <= 1e-13 * sf2 * max(1.0, 1.0 / ell ** 2)
        assert ref[0, 0] == sf2


@pytest.mark.parametrize("family", R.GRAD_FAMILIES)
@pytest.mark.parametrize("ell", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("point_major", [0, 1])
def test_gradient_blocks_against_the_oracle(family, ell, point_major):
    rng = np.random.default_rng(10 + family)
    for d in (1, 3, 7):
        N, M, pt = 11, 5, d + 1
        X, Z = R.grid_points(rng, N, d), R.grid_points(rng, M, d)
        Z[0] = X[0]
        sf2 = 1.5
        V, T, ND = R.grad_blocks(family, X, Z, 1.0 / ell, sf2)
        got = R.as_rows(V, pt, point_major)                                          # rows (j, q) by point_major, columns i·pt + q'
        # the oracle: rows (q', i) over the training points, columns (q, j) over the candidates, both by outputs
        orc = GO.grad_kernel_matrix(family, ell, sf2, X, Z).reshape(pt, N, pt, M)     # [q'][i][q][j]
        j, q = R.row_index(M, pt, point_major)
        want = orc.transpose(3, 2, 1, 0)[j, q].reshape(M * pt, N * pt)                # [j][q][i][q'] → rows, point-major columns
        assert np.max(np.abs(got - want)) <= 1e-13 * sf2 * max(1.0, 1.0 / ell ** 2)
        assert ND[0, 0] == 0 and ND[0, 1] == 1 and ND[1, 0] == 1 and ND[pt - 1, pt - 1] == 2
        assert np.all(T >= 0) and np.all(np.abs(V) <= sf2 * max(1.0, 1.0 / ell ** 2) * T * (1 + 1e-15))


@pytest.mark.parametrize("family", R.GRAD_FAMILIES)
@pytest.mark.parametrize("ell", [1.0, 0.5, 2.0])
def test_dlogell_blocks_against_a_central_difference(family, ell):
    rng = np.random.default_rng(20 + family)
    d, N, M = 3, 9, 6
    X, Z = R.grid_points(rng, N, d), R.grid_points(rng, M, d)
    Z[0] = X[0]
    D, T, _ = R.grad_blocks(family, X, Z, 1.0 / ell, 1.5, dlogell=True)
    h = np.longdouble(1e-4)
    Vp, _, _ = R.grad_blocks(family, X, Z, 1.0 / ell, 1.5, ell_scale=np.exp(h))
    Vm, _, _ = R.grad_blocks(family, X, Z, 1.0 / ell, 1.5, ell_scale=np.exp(-h))
    fd = (Vp - Vm) / (2 * h)
    pt = d + 1
    for q in range(pt):
        for qp in range(pt):
            blk, ref = D[:, q, :, qp], fd[:, q, :, qp]
            assert np.max(np.abs(blk - ref)) <= 1e-7 * np.max(np.abs(ref)), (q, qp)
    assert np.all(np.abs(D) <= 1.5 * max(1.0, 1.0 / ell ** 2) * T * (1 + 1e-15))


def test_plane_offset_is_injective_and_inside_the_plane():
    Mc, res_ld = 272, 640
    res_plane = R.pad_up(Mc, 256) * res_ld
    j, k = np.meshgrid(np.arange(Mc), np.arange(res_ld), indexing="ij")
    off = R.plane_offset(j, k, res_ld).reshape(-1)
    assert off.min() == 0 and off.max() + 1 <= res_plane
    assert np.unique(off).size == off.size
    # the library's own statement of the layout (csrc/abo_oz_dev.h: block (R, H) of 256 rows × 64 bytes at ((R·nhs) + H)·16384)
    want = ((j >> 8) * (res_ld // 64) + (k >> 6)) * 16384 + (j & 255) * 64 + (k & 63)
    np.testing.assert_array_equal(off, want.reshape(-1))


def test_residues_are_signed_bytes_congruent_to_the_value():
    rng = np.random.default_rng(3)
    x = np.rint(rng.uniform(-2.0 ** 52, 2.0 ** 52, 2000))
    x[:3] = [0.0, -1.0, 2.0 ** 52 - 1]
    for n in (8, 9, 10, 14):
        r = R.residues(x, n)
        assert r.dtype == np.int8 and r.shape == (n, x.size)
        for l, p in enumerate(R.moduli(n)):
            assert all((int(v) - int(b)) % p == 0 for v, b in zip(x[:200], r[l][:200]))
            assert p == 256 or np.max(np.abs(r[l].astype(np.int64))) <= (p - 1) // 2


def test_every_gpu_input_set_has_an_exact_r2():
    names = set()
    for name, X, Z, s in R.input_sets():
        assert name not in names
        names.add(name)
        r2 = R.assert_exact_r2(X, Z, s, pairs=24, seed=len(names))
        assert r2.shape == (Z.shape[0], X.shape[0]) and r2[0, 0] == 0.0 and r2[-1, -1] == 0.0       # the coincident candidates
        assert np.max(r2) <= 280.0
    assert len(names) == 2 * len(R.STD_DIMS) + 4 + 4 * len(R.GRAD_DIMS)


def test_abo_test_kgen_args_layout_matches_the_header():
    import ctypes as C
    from abstractbayesopt.jl_amd._lib import AboTestKgenArgs as A
    assert C.sizeof(A) == 5 * 8 + 3 * 8 + 6 * 4 + 2 * 8 + 8 + 6 * 4 + 8 + 2 * 8 + 8 + 4 * 4
    assert A.ldk.offset == 40 and A.Mc.offset == 64 and A.s.offset == 88 and A.mean_vec.offset == 104 and A.pt.offset == 112
    assert A.res.offset == 136 and A.res_bad.offset == 160 and A.res_n.offset == 168
