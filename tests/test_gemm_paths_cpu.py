"""Host-side decisions of the fp64 MFMA GEMM family (csrc/gemm.hip), no GPU needed: the workgroup → tile map of the swizzled SYRK
launch (gemm_swz_q / gemm_swz_tile, the very functions gemm_nt_kernel calls) and the launcher's choice of kernel (gemm_nt_path, the one
function launch_gemm_nt switches on), through the host-only hooks abo_test_gemm_swz_q, abo_test_gemm_swz_map and abo_test_gemm_path of
the test build.  What the chosen kernels compute is tests/test_gpu_gemm_family.py."""
import ctypes as C

import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import (GEMM_PATH_SKINNY as SKINNY, GEMM_PATH_SMALL as SMALL, GEMM_PATH_SPLITK as SPLITK,
                                          GEMM_PATH_SWIZZLED as SWIZZLED, GEMM_PATH_TILED as TILED, K_A_LOWER, K_B_LOWER, K_FULL)


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    monkeypatch.delenv("ABO_GEMM_SMALL", raising=False)
    monkeypatch.delenv("ABO_GEMM_NO_SWIZZLE", raising=False)


def swz_tile(T, G, Q):
    ti, tj = C.c_int32(-1), C.c_int32(-1)
    abo._lib.check(abo._lib.lib().abo_test_gemm_swz_map(T, G, Q, C.byref(ti), C.byref(tj)))
    return ti.value, tj.value


def swz_q(tiles, L):
    q = C.c_int32(-1)
    abo._lib.check(abo._lib.lib().abo_test_gemm_swz_q(tiles, L, C.byref(q)))
    return q.value


def path(M, N, K, kmode=K_FULL, lower_only=0, batch=1, ksplit=0, mrows=0, in_place=0):
    p = C.c_int32(-99)
    abo._lib.check(abo._lib.lib().abo_test_gemm_path(M, N, K, kmode, lower_only, batch, ksplit, mrows, in_place, C.byref(p)))
    return p.value


# ---- the swizzled map --------------------------------------------------------------------------------------------------------------
SWZ_CASES = [(T, 4) for T in range(1, 65)] + [(T, G) for G in (1, 2, 3, 8) for T in (1, 2, 7, 8, 9, 16, 17, 18, 19, 23, 37)]


@pytest.mark.parametrize("T,G", SWZ_CASES)
def test_swizzled_map_hits_every_lower_tile_exactly_once(T, G):
    """A tile the map misses keeps its old value, a tile it hits twice is updated twice: the images of Q = 0 … T(T+1)/2 − 1 are the
    lower tiles, each once — whatever the number of rows (0 … G − 1) the last super-row is short of G."""
    tiles = T * (T + 1) // 2
    images = [swz_tile(T, G, Q) for Q in range(tiles)]
    assert sorted(images) == [(ti, tj) for ti in range(T) for tj in range(ti + 1)]


@pytest.mark.parametrize("T,G", SWZ_CASES)
def test_swizzled_map_walks_super_rows_of_G_tile_rows_in_order(T, G):
    """the locality the map exists for: the sequence finishes one super-row of G tile rows before it enters the next"""
    supers = [swz_tile(T, G, Q)[0] // G for Q in range(T * (T + 1) // 2)]
    assert supers == sorted(supers)


@pytest.mark.parametrize("T", list(range(1, 65)))
def test_xcd_interleave_of_the_padded_grid_is_a_bijection_onto_the_tile_sequence(T):
    """workgroup L of the ⌈tiles/8⌉·8 launched: every position Q < tiles is taken by exactly one L, every other L idles (Q ≥ tiles)"""
    tiles = T * (T + 1) // 2
    grid = (tiles + 7) // 8 * 8
    qs = [swz_q(tiles, L) for L in range(grid)]
    assert sorted(q for q in qs if q < tiles) == list(range(tiles))
    assert len([q for q in qs if q >= tiles]) == grid - tiles
    per = grid // 8
    assert all(qs[L] // per == L % 8 for L in range(grid))          # XCD L % 8 (round-robin dispatch) owns the (L % 8)-th eighth


def test_full_workgroup_to_tile_map_of_the_production_launch():
    """L → Q → (ti, tj) end to end at the tile counts of the swizzled GPU cases (G = 4, last super-rows of 0, 1, 2, 3 rows)"""
    for T in (16, 17, 18, 19):
        tiles = T * (T + 1) // 2
        hit = [swz_tile(T, 4, q) for q in (swz_q(tiles, L) for L in range((tiles + 7) // 8 * 8)) if q < tiles]
        assert sorted(hit) == [(ti, tj) for ti in range(T) for tj in range(ti + 1)]


def test_swizzled_map_hooks_refuse_what_lies_outside_the_map():
    lib = abo._lib.lib()
    ti, tj, q = C.c_int32(), C.c_int32(), C.c_int32()
    for T, G, Q in [(0, 4, 0), (4, 0, 0), (4, 4, -1), (4, 4, 10)]:
        assert lib.abo_test_gemm_swz_map(T, G, Q, C.byref(ti), C.byref(tj)) == abo._lib.ABO_EINVAL
    assert lib.abo_test_gemm_swz_map(4, 4, 0, None, C.byref(tj)) == abo._lib.ABO_EINVAL
    for tiles, L in [(0, 0), (10, -1), (10, 16)]:
        assert lib.abo_test_gemm_swz_q(tiles, L, C.byref(q)) == abo._lib.ABO_EINVAL


# ---- the launcher's choice ------------------------------------------------------------------------------------------------------------
T_ = 128      # tile edge


@pytest.mark.parametrize("kw,want", [
    # the small kernel takes launches of at most 64 tiles …
    (dict(M=8 * T_, N=8 * T_, K=128), SMALL),                                  # 64 tiles
    (dict(M=5 * T_, N=13 * T_, K=128), TILED),                                 # 65
    (dict(M=T_, N=T_, K=128, batch=64), SMALL),                                # the batch multiplies the count
    (dict(M=T_, N=T_, K=128, batch=65), TILED),
    # … whose K is a multiple of 128 …
    (dict(M=T_, N=T_, K=112), TILED),
    (dict(M=T_, N=T_, K=128), SMALL),
    (dict(M=2 * T_, N=3 * T_, K=272), TILED),
    (dict(M=2 * T_, N=3 * T_, K=384), SMALL),
    # … and whose C is neither operand
    (dict(M=T_, N=T_, K=128, in_place=1), TILED),
    # lower_only counts the tiles (ti, tj ≤ ti), tj < Tn
    (dict(M=11 * T_, N=11 * T_, K=128), TILED),                                # 121
    (dict(M=11 * T_, N=11 * T_, K=128, lower_only=1), TILED),                  # 66
    (dict(M=10 * T_, N=10 * T_, K=128, lower_only=1), SMALL),                  # 55
    (dict(M=11 * T_, N=8 * T_, K=128, lower_only=1), SMALL),                   # Tm > Tn: 36 + 3·8 = 60
    (dict(M=12 * T_, N=8 * T_, K=128, lower_only=1), TILED),                   # 36 + 4·8 = 68
    (dict(M=11 * T_, N=8 * T_, K=128), TILED),                                 # 88 without lower_only
    (dict(M=8 * T_, N=20 * T_, K=128, lower_only=1), SMALL),                   # Tm < Tn: 36
    (dict(M=8 * T_, N=20 * T_, K=128), TILED),                                 # 160
    (dict(M=4 * T_, N=4 * T_, K=128, lower_only=1, batch=6), SMALL),           # 10 · 6 = 60
    (dict(M=4 * T_, N=4 * T_, K=128, lower_only=1, batch=7), TILED),           # 70
    # the swizzled launch: square, lower_only, K_FULL, one batch, at least 16 tile rows
    (dict(M=15 * T_, N=15 * T_, K=128, lower_only=1), TILED),
    (dict(M=16 * T_, N=16 * T_, K=128, lower_only=1), SWIZZLED),
    (dict(M=16 * T_, N=16 * T_, K=32, lower_only=1), SWIZZLED),
    (dict(M=19 * T_, N=19 * T_, K=32, lower_only=1, in_place=1), SWIZZLED),
    (dict(M=16 * T_, N=16 * T_, K=128, lower_only=0), TILED),
    (dict(M=16 * T_, N=16 * T_, K=128, lower_only=1, kmode=K_A_LOWER), TILED),
    (dict(M=16 * T_, N=16 * T_, K=128, lower_only=1, batch=2), TILED),
    (dict(M=17 * T_, N=16 * T_, K=128, lower_only=1), TILED),
    (dict(M=16 * T_, N=17 * T_, K=128, lower_only=1), TILED),
])
def test_path_by_the_rule(kw, want):
    assert path(**kw) == want


@pytest.mark.parametrize("env,kw,want", [
    ("0", dict(M=T_, N=T_, K=128), TILED),                                     # 0: never the small kernel
    ("0", dict(M=16 * T_, N=16 * T_, K=128, lower_only=1), SWIZZLED),
    ("1", dict(M=16 * T_, N=16 * T_, K=128), SMALL),                           # 1: always, where it can run at all …
    ("1", dict(M=16 * T_, N=16 * T_, K=128, lower_only=1), SMALL),             # … in front of the swizzled launch too
    ("1", dict(M=16 * T_, N=16 * T_, K=112), TILED),
    ("1", dict(M=16 * T_, N=16 * T_, K=128, in_place=1), TILED),
    ("1", dict(M=T_, N=3 * T_, K=384, ksplit=128), SPLITK),                    # split-k has no small form
    ("1", dict(M=T_, N=3 * T_, K=384, ksplit=128, mrows=16), SKINNY),
])
def test_path_under_ABO_GEMM_SMALL(monkeypatch, env, kw, want):
    monkeypatch.setenv("ABO_GEMM_SMALL", env)
    assert path(**kw) == want


def test_path_under_ABO_GEMM_NO_SWIZZLE(monkeypatch):
    kw = dict(M=16 * T_, N=16 * T_, K=128, lower_only=1)
    assert path(**kw) == SWIZZLED
    monkeypatch.setenv("ABO_GEMM_NO_SWIZZLE", "1")
    assert path(**kw) == TILED
    assert path(M=T_, N=T_, K=128) == SMALL                                    # nothing else changes
    monkeypatch.delenv("ABO_GEMM_NO_SWIZZLE")
    assert path(**kw) == SWIZZLED


@pytest.mark.parametrize("M", [128, 256])
@pytest.mark.parametrize("mrows", [0, 16, 24, 32, 48, 64, 80])
def test_split_k_path(M, mrows):
    """the skinny kernel serves M = 128 with 16, 32, 48 or 64 live rows; everything else runs the tiled kernel chunk by chunk"""
    want = SKINNY if (M == 128 and mrows in (16, 32, 48, 64)) else SPLITK
    for kmode in (K_FULL, K_B_LOWER):
        assert path(M=M, N=384, K=384, kmode=kmode, ksplit=128, mrows=mrows) == want
        assert path(M=M, N=384, K=384, kmode=kmode, ksplit=256, mrows=mrows, in_place=1) == want


def test_path_hook_refuses_what_the_kernels_cannot_run():
    lib = abo._lib.lib()
    p = C.c_int32(-99)
    ok = dict(M=128, N=128, K=128, kmode=0, lower_only=0, batch=1, ksplit=0, mrows=0, in_place=0)
    for bad in (dict(M=0), dict(M=100), dict(N=192), dict(K=0), dict(K=24), dict(kmode=5), dict(kmode=-1), dict(batch=0), dict(ksplit=64),
                dict(ksplit=128, batch=2), dict(ksplit=128, K=144), dict(ksplit=-128), dict(mrows=-16)):
        a = dict(ok, **bad)
        st = lib.abo_test_gemm_path(a["M"], a["N"], a["K"], a["kmode"], a["lower_only"], a["batch"], a["ksplit"], a["mrows"], a["in_place"],
                                    C.byref(p))
        assert st == abo._lib.ABO_EINVAL, bad
        assert p.value == -99
    assert lib.abo_test_gemm_path(128, 128, 128, 0, 0, 1, 0, 0, 0, None) == abo._lib.ABO_EINVAL


# ---- the references of tests/test_gpu_gemm_family.py are exact -------------------------------------------------------------------------
def test_the_integer_operands_keep_the_numpy_references_exact():
    """The GPU file compares with equality: its fp64 numpy references must be the true integers.  Recomputed in int64 at the largest k
    of that file, with every kmode, and for the variance contraction at its largest Np."""
    import numpy as np

    from tests import gemm_family_ref as R
    rng = np.random.default_rng(1)
    M, N, K = 256, 384, 384
    A, B = R.padded(rng, M, K, K + 6, 64), R.padded(rng, N, K, K + 2, 64)
    for kmode in range(5):
        f, i = R.acc_ref(A, B, M, N, K, kmode), R.acc_ref(A, B, M, N, K, kmode, dtype=np.int64)
        assert i.dtype == np.int64 and np.array_equal(f, i.astype(np.float64)) and np.abs(i).max() < 2 ** 30
        for alpha in R.ALPHAS:
            for beta in R.BETAS:
                v = alpha * f + beta * 64.0                       # exact: one binary digit behind the point at most
                assert np.array_equal(v * 2, np.round(v * 2)) and np.abs(v).max() < 2 ** 31
    assert not np.array_equal(R.acc_ref(A, B, M, N, K, R.K_A_LOWER), R.acc_ref(A, B, M, N, K, R.K_FULL))      # dense: the range shows
    assert not np.array_equal(R.acc_ref(A, B, M, N, K + 2, R.K_FULL), R.acc_ref(A, B, M, N, K, R.K_FULL))     # so does the sentinel
    parts = [R.acc_ref(A, B, M, N, K, R.K_B_LOWER, chunk=(z * 256, (z + 1) * 256)) for z in range(2)]
    assert np.isnan(parts[1][:, :256]).all() and not np.isnan(parts[1][:, 256:]).any() and not np.isnan(parts[0]).any()
    assert np.array_equal(parts[0] + np.nan_to_num(parts[1]), R.acc_ref(A, B, M, N, K, R.K_B_LOWER))
    Np, Mc = 768, 256
    W, Kxz = R.tri_w(rng, Np, Np + 6), R.padded(rng, Mc, Np, Np + 2, 8, nonzero=True)
    assert np.all(np.triu(W[:, :Np], 1) == 0) and np.all(np.tril(W[:, :Np]) [np.tril_indices(Np)] != 0)
    for nvalid in (Np, Np - 129, Np - 255):
        f, i = R.var_ref(W, Kxz, Np, Mc, nvalid), R.var_ref(W, Kxz, Np, Mc, nvalid, dtype=np.int64)
        assert np.array_equal(f, i.astype(np.float64)) and i.max() < 2 ** 40
    assert np.array_equal(R.var_ref(W, Kxz, Np, Mc, Np), R.var_ref(W, Kxz, Np, Mc, Np, block_range=True))     # triangular W: same thing
    assert np.all(R.var_ref(W, Kxz, Np, Mc, Np - 129)[-1] == 0) and np.any(R.var_ref(W, Kxz, Np, Mc, Np - 127)[-1] != 0)
