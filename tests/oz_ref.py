"""Plain references for the stages of the int8 residue engine (csrc/ozaki.hip), in numpy and Python integers — TEST INFRASTRUCTURE ONLY.

What tests/test_gpu_oz_family.py holds the kernels against: the two device layouts (residue planes: oz_plane_off; residue products:
oz_u_block) as pack / unpack pairs, the nearest symmetric residue, the row-scale rule, the guard of the short plan and the exact
Chinese-remainder reconstruction.  The plan constants and the moduli are oracle/ozaki_oracle.py's.  Each evaluator is pinned against
brute force by tests/test_oz_ref_cpu.py."""
import math

import numpy as np

from oracle.ozaki_oracle import moduli, plan                                   # noqa: F401  (re-exported)
from tests.test_prune_shortplan_cpu import bound_kbits, guard_delta, k_scale, pow2   # noqa: F401  the guard δ_i of the short plan, exact rationals

T = 256                      # tile edge (OZ_T)
SEXP_MAX = 960               # oz_row_scale's clamp (OZ_SEXP_MAX)
SEXP_BAD = -(1 << 20)        # the row scale of a row whose norm is not finite or ≥ 1e300 (OZ_SEXP_BAD)
FULL_KBITS = 53


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def plane_off(row, k, nhs):
    """oz_plane_off: blocks of 256 rows × 64 k-bytes, row-major inside a block, block (R, H) at (R·nhs + H)·16 KiB"""
    return ((row >> 8) * nhs + (k >> 6)) * 16384 + (row & 255) * 64 + (k & 63)


def plane_pack(a, ld, fill=0x5A):
    """a [rows][cols] int8 (rows a multiple of 256, cols ≤ ld, ld a multiple of 64) → the plane's rows·ld bytes in the device layout;
    bytes k ≥ cols of a row keep `fill`"""
    a = np.asarray(a, dtype=np.int8)
    rows, cols = a.shape
    assert rows % 256 == 0 and ld % 64 == 0 and cols <= ld
    full = np.full((rows, ld), fill, dtype=np.uint8).view(np.int8)
    full[:, :cols] = a
    # [R][256][nhs][64] → [R][nhs][256][64]
    return np.ascontiguousarray(full.reshape(rows // 256, 256, ld // 64, 64).transpose(0, 2, 1, 3)).reshape(-1)


def plane_unpack(buf, rows, cols, ld):
    """the [rows][cols] view of a plane of row stride ld"""
    buf = np.asarray(buf).view(np.int8).reshape(-1)[:rows * ld]
    return buf.reshape(rows // 256, ld // 64, 256, 64).transpose(0, 2, 1, 3).reshape(rows, ld)[:, :cols]


def u_off(i, j, l, Ti, n):
    """oz_u_block + the position inside the 64 KiB block: [256 rows i][256 candidates j]"""
    return (((j >> 8) * Ti + (i >> 8)) * n + l) * (T * T) + (i & 255) * T + (j & 255)


def u_pack(U):
    """U [n][256·Ti][256·Tj] int8 → the device buffer: blocks [tj][ti][l] of [256][256]"""
    U = np.asarray(U, dtype=np.int8)
    n, R, Cc = U.shape
    assert R % T == 0 and Cc % T == 0
    return np.ascontiguousarray(U.reshape(n, R // T, T, Cc // T, T).transpose(3, 1, 0, 2, 4)).reshape(-1)


def u_unpack(buf, n, Ti, Tj):
    buf = np.asarray(buf).view(np.int8).reshape(-1)[:n * Ti * Tj * T * T]
    return buf.reshape(Tj, Ti, n, T, T).transpose(2, 1, 3, 0, 4).reshape(n, Ti * T, Tj * T)


# ---- residues --------------------------------------------------------------------------------------------------------------------------
def residues(x, p):
    """the nearest symmetric representative of x mod p as a signed byte: r = x % p (Python's: 0 ≤ r < p), minus p where 2r ≥ p — for odd
    p the range [−(p−1)/2, (p−1)/2], for p = 256 the byte of x: 128 is −128.  x: Python integers, an object array of them, or int64."""
    x = np.asarray(x)
    if x.dtype == object:
        r = np.array([int(v) % p for v in x.reshape(-1)], dtype=np.int64).reshape(x.shape)
    else:
        r = np.mod(x.astype(np.int64), p)                       # floor modulo, as Python's %
    return np.where(2 * r >= p, r - p, r).astype(np.int8)


def quantise(x, s):
    """rint(x·2^s) as int64 (exact scaling, ties to even as the device rounds); |result| must stay below 2^63"""
    return np.rint(np.ldexp(np.asarray(x, dtype=np.float64), s)).astype(np.int64)


# ---- the row-scale rule ----------------------------------------------------------------------------------------------------------------
def row_scale(l1, mx, eP, kbits, ktg=0):
    """oz_rowscale_kernel through math.frexp: s = min(eP − kbits − e(L1), 52 − e(max), SEXP_MAX − max(ktg, 0)); 0 for an all-zero row;
    SEXP_BAD where the norm is not finite or ≥ 1e300"""
    if mx == 0.0 and l1 == 0.0:
        return 0
    if not (mx > 0.0 and l1 < 1.0e300):
        return SEXP_BAD
    return min(eP - kbits - math.frexp(l1)[1], 52 - math.frexp(mx)[1], SEXP_MAX - max(ktg, 0))


def rec_bound(n, eP):
    """(128n² + 256n)·2^(eP−91): the reconstruction's fp64 error in units of the integer image (ozaki.hip: "the guarded bound")"""
    return (128.0 * n * n + 256.0 * n) * 2.0 ** (eP - 91)


# ---- exact reconstruction --------------------------------------------------------------------------------------------------------------
def crt_weights(n):
    pl = plan(n)
    P = pl["P"]
    return P, [(P // p) * pow(P // p, -1, p) for p in pl["p"]]


def crt_exact(U):
    """U [n][...] residues (any representative) → the integers C ≡ U_l (mod p_l) in (−P/2, P/2], an object array of Python integers"""
    U = np.asarray(U)
    n = U.shape[0]
    P, w = crt_weights(n)
    flat = U.reshape(n, -1)
    out = np.empty(flat.shape[1], dtype=object)
    for e in range(flat.shape[1]):
        c = sum(int(flat[l, e]) * w[l] for l in range(n)) % P
        out[e] = c - P if 2 * c > P else c
    return out.reshape(U.shape[1:])


def residues_of(C, n):
    """the residue bytes [n][...] of an (object) array of integers"""
    C = np.asarray(C, dtype=object)
    return np.stack([residues(C, p) for p in plan(n)["p"]])


# ---- the tile list of the persistent GEMM ----------------------------------------------------------------------------------------------
def launch_shape(Ti, Tj, n):
    """(tjg, ngi, ngj, blocks) as launch_oz_gemm derives them"""
    tjg = 64 if Tj >= 64 else -(-Tj // 8) * 8
    ngi, ngj = (Ti + 3) // 4, -(-Tj // tjg)
    return tjg, ngi, ngj, ngi * n * ngj * 4 * tjg
