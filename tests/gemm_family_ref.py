"""Inputs and plain numpy references for the direct tests of the fp64 MFMA GEMM family (tests/test_gpu_gemm_family.py; the exactness
check of the references themselves runs without a GPU: tests/test_gemm_paths_cpu.py).

Every operand is INTEGER-valued fp64.  GEMM operands lie in [−64, 64]: with K ≤ 4096 every product (≤ 2¹²) and every partial sum
(≤ 2¹²·2¹² = 2²⁴) stays far below 2⁵³, alpha, beta ∈ {1, −1, −1.5, 0.5, 0} keep one binary digit behind the point at most, so every
summation order — the kernels' MFMA order, numpy's, int64's — gives the same bits and every comparison is an equality.  The variance
operands lie in [−8, 8]: |V| ≤ 64·Np < 2¹⁶ for Np ≤ 1024, V² < 2³², a 128-row block sum < 2³⁹."""
import numpy as np

K_FULL, K_A_LOWER, K_A_UPPER, K_B_LOWER, K_B_UPPER = range(5)
TB = 128
SENTINEL = float(2 ** 40)          # fills the padding behind a row's logical width: one element read from there shows in the result
ALPHAS = (1.0, -1.0, -1.5, 0.5, 0.0)
BETAS = (1.0, -1.0, -1.5, 0.5)      # the non-zero ones


def ints(rng, shape, lim):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def padded(rng, rows, width, ld, lim, fill=SENTINEL, nonzero=False):
    """[rows][ld] with integer entries of magnitude ≤ lim in the first `width` columns and `fill` behind them"""
    a = np.full((rows, ld), fill, dtype=np.float64)
    v = ints(rng, (rows, width), lim)
    if nonzero:
        v[v == 0.0] = 1.0
    a[:, :width] = v
    return a


def krange(kmode, ti, tj, K):
    """the kernels' stated contract: the k range of tile (ti, tj) at 128-block granularity, clipped to K"""
    kb, ke = 0, K
    if kmode == K_A_LOWER:
        ke = min(K, (ti + 1) * TB)
    elif kmode == K_A_UPPER:
        kb = min(K, ti * TB)
    elif kmode == K_B_LOWER:
        ke = min(K, (tj + 1) * TB)
    elif kmode == K_B_UPPER:
        kb = min(K, tj * TB)
    return kb, ke


def acc_ref(A, B, M, N, K, kmode, chunk=None, dtype=np.float64):
    """acc[i][j] = Σ_{k in range(tile of (i, j))} A[i][k]·B[j][k].  chunk = (k0, k1): the split-k partial of that chunk — the range is
    intersected with it, and a tile whose intersection is empty is NaN (nothing is written there); chunk = None: an empty range is a
    zero (the plain kernels write alpha·0 + beta·C)."""
    out = np.full((M, N), np.nan if chunk is not None else 0.0, dtype=np.float64 if chunk is not None else dtype)
    Ai, Bi = A[:M, :K].astype(dtype), B[:N, :K].astype(dtype)
    for ti in range((M + TB - 1) // TB):
        for tj in range((N + TB - 1) // TB):
            kb, ke = krange(kmode, ti, tj, K)
            if chunk is not None:
                kb, ke = max(kb, chunk[0]), min(ke, chunk[1])
                if kb >= ke:
                    continue
            out[ti * TB:(ti + 1) * TB, tj * TB:(tj + 1) * TB] = Ai[ti * TB:(ti + 1) * TB, kb:ke] @ Bi[tj * TB:(tj + 1) * TB, kb:ke].T
    return out


def lower_mask(M, N):
    """True on the tiles with tj ≤ ti: what a lower_only launch writes"""
    ti = np.arange(M)[:, None] // TB
    tj = np.arange(N)[None, :] // TB
    return tj <= ti


def tri_w(rng, Np, ldw, lim=8):
    """lower-triangular W [Np][ldw]: non-zero integers on and below the diagonal, exact zeros above it, the sentinel behind column Np"""
    W = padded(rng, Np, Np, ldw, lim, nonzero=True)
    W[:, :Np] = np.tril(W[:, :Np])
    return W


def var_ref(W, Kxz, Np, Mc, nvalid, block_range=False, dtype=np.float64):
    """partial[tb][j] = Σ_{i in 128-row block tb, i < nvalid} V[i][j]², V = W·Kxzᵀ over k < Np — or, block_range: over k < (tb+1)·128 for
    the rows of block tb (what the 128-row kernel reads of a W that is not triangular)"""
    Wi, Ki = W[:Np, :Np].astype(dtype), Kxz[:Mc, :Np].astype(dtype)
    out = np.zeros((Np // TB, Mc), dtype=dtype)
    for tb in range(Np // TB):
        ke = (tb + 1) * TB if block_range else Np
        V = Wi[tb * TB:(tb + 1) * TB, :ke] @ Ki[:, :ke].T
        V[max(0, min(TB, nvalid - tb * TB)):, :] = 0
        out[tb] = (V * V).sum(axis=0)
    return out
