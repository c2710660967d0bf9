"""tests/oz_ref.py against brute force on small cases, and the residue GEMM's ticket decode (abo_test_oz_tickets: host only) against its
contract: every tile of a launch exactly once, whatever the shape.  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo

from tests import oz_ref as R


def test_plane_layout_round_trip_and_offsets():
    rng = np.random.default_rng(1)
    a = rng.integers(-128, 128, (512, 192), dtype=np.int8)
    buf = R.plane_pack(a, 192)
    np.testing.assert_array_equal(R.plane_unpack(buf, 512, 192, 192), a)
    for r, k in [(0, 0), (1, 0), (0, 63), (0, 64), (255, 191), (256, 0), (511, 130)]:           # oz_plane_off, written out
        off = ((r // 256) * 3 + k // 64) * 16384 + (r % 256) * 64 + k % 64
        assert buf[off] == a[r, k] and R.plane_off(r, k, 3) == off
    assert sorted(set(R.plane_off(*np.meshgrid(np.arange(512), np.arange(192), indexing="ij"), 3).ravel())) == list(range(512 * 192))
    # the bound pass's layout: 256 written columns in planes that keep a row stride of 768
    b = rng.integers(-128, 128, (256, 256), dtype=np.int8)
    wide = R.plane_pack(b, 768)
    assert wide.size == 256 * 768
    np.testing.assert_array_equal(R.plane_unpack(wide, 256, 256, 768), b)
    rest = np.ones(wide.size, bool)
    rest[R.plane_off(*np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), 12).ravel()] = False
    assert np.all(wide.view(np.uint8)[rest] == 0x5A) and rest.sum() == 256 * 512


def test_u_layout_round_trip_and_offsets():
    rng = np.random.default_rng(2)
    U = rng.integers(-128, 128, (9, 512, 768), dtype=np.int8)
    buf = R.u_pack(U)
    np.testing.assert_array_equal(R.u_unpack(buf, 9, 2, 3), U)
    for l, i, j in [(0, 0, 0), (8, 511, 767), (3, 256, 255), (5, 255, 256), (1, 300, 700)]:       # oz_u_block, written out
        off = (((j // 256) * 2 + i // 256) * 9 + l) * 65536 + (i % 256) * 256 + j % 256
        assert buf[off] == U[l, i, j] and R.u_off(i, j, l, 2, 9) == off


def test_residues_are_the_nearest_symmetric_representative():
    for p in R.moduli(16):
        xs = list(range(-3 * p, 3 * p + 1)) + [2 ** 52 - 1, -(2 ** 52), 2 ** 62 + 12345, -(2 ** 30), 2 ** 30]
        want = []
        for x in xs:                                                    # brute force: the representative of least magnitude
            c = [r for r in range(-128, 128) if (x - r) % p == 0]
            m = min(abs(r) for r in c)
            want.append(min(r for r in c if abs(r) == m))              # the tie (p = 256: ±128) goes to −128, the byte
        np.testing.assert_array_equal(R.residues(np.array(xs, dtype=np.int64), p), want)
        np.testing.assert_array_equal(R.residues(np.array(xs, dtype=object), p), want)
    assert R.residues(np.array([128, 384, -128]), 256).tolist() == [-128, -128, -128]
    big = np.array([3 ** 70, -(3 ** 70)], dtype=object)
    assert [int(v) for v in R.residues(big, 251)] == [((3 ** 70 + 125) % 251) - 125, ((-(3 ** 70) + 125) % 251) - 125]


def test_row_scale_and_quantise():
    assert R.row_scale(1.0, 1.0, 108, 53) == min(108 - 53 - 1, 52 - 1)
    assert R.row_scale(math.nextafter(1.0, 0.0), 2.0 ** -10, 108, 53) == 108 - 53 - 0   # one ulp below a power of two: e(L1) = 0 …
    assert R.row_scale(1.0, 2.0 ** -10, 108, 53) == 108 - 53 - 1                         # … and exactly at it: e(L1) = 1
    assert R.row_scale(3.0, 3.0, 61, 25) == 61 - 25 - 2
    assert R.row_scale(2.0 ** -1040, 2.0 ** -1041, 108, 53) == R.SEXP_MAX and R.row_scale(2.0 ** -1040, 2.0 ** -1041, 108, 53, 7) == R.SEXP_MAX - 7
    assert R.row_scale(0.0, 0.0, 108, 53) == 0
    for l1, mx in [(float("nan"), 1.0), (float("inf"), float("inf")), (1e300, 5e299), (2e300, 1e299)]:
        assert R.row_scale(l1, mx, 108, 53) == R.SEXP_BAD
    np.testing.assert_array_equal(R.quantise([0.5, 1.5, 2.5, -0.5, -1.5, -0.0, 0.75], 0), [0, 2, 2, 0, -2, 0, 1])      # ties to even
    np.testing.assert_array_equal(R.quantise([(2 ** 52 - 1) * 2.0 ** -52, 1.0 - 2.0 ** -53], 52), [2 ** 52 - 1, 2 ** 52])       # the second: a tie, to even


@pytest.mark.parametrize("n", [8, 12, 14, 16])
def test_crt_exact_inverts_the_residues(n):
    rng = np.random.default_rng(n)
    P = R.plan(n)["P"]
    C0 = [0, 1, -1, P // 2, -(P // 2) + 1 if P % 2 == 0 else -(P // 2), P // 4 - 1, -(P // 4)] + \
        [int(rng.integers(-2 ** 62, 2 ** 62)) * int(rng.integers(1, 2 ** 40)) % (P // 2) for _ in range(20)]
    Cs = np.array(C0, dtype=object)
    U = R.residues_of(Cs, n)
    assert U.shape == (n, len(C0)) and U.dtype == np.int8
    assert list(R.crt_exact(U)) == C0
    assert all(-P // 2 < c <= P // 2 for c in R.crt_exact(rng.integers(-128, 128, (n, 50))))


# ---- the ticket decode ----------------------------------------------------------------------------------------------------------------
def tickets(Ti, Tj, n):
    L = abo._lib.lib()
    cnt = C.c_int64(-1)
    abo._lib.check(L.abo_test_oz_tickets(Ti, Tj, n, None, C.byref(cnt)))
    tiles = np.empty(cnt.value, dtype=np.int32)
    abo._lib.check(L.abo_test_oz_tickets(Ti, Tj, n, tiles.ctypes.data, C.byref(cnt)))
    return tiles, cnt.value


def assert_every_tile_once(Ti, Tj, n):
    tiles, blocks = tickets(Ti, Tj, n)
    tjg, ngi, ngj, want_blocks = R.launch_shape(Ti, Tj, n)
    assert blocks == want_blocks and blocks % 8 == 0 and tiles.size == blocks            # 8·per_list is the launcher's `blocks`
    real = tiles[tiles >= 0].astype(np.int64)
    assert np.all(tiles[tiles < 0] == -1) and real.size == Ti * Tj * n
    ti, tj, l = real & 511, (real >> 9) & 2047, real >> 20                                 # as the kernel unpacks them
    assert ti.max() < Ti and tj.max() < Tj and l.max() < n
    assert np.all(np.bincount((l * Ti + ti) * Tj + tj, minlength=Ti * Tj * n) == 1)       # the set {(ti, tj, l)}, each once
    return blocks


@pytest.mark.parametrize("n", [8, 14, 16])
def test_ticket_decode_takes_every_tile_exactly_once(n):
    for Ti in range(1, 41):
        for Tj in range(1, 131):
            assert_every_tile_once(Ti, Tj, n)


def test_ticket_decode_at_the_largest_launch_the_engine_offers():
    """The engine's limits, read from posterior.hip: wants_int8 offers the engine up to Np = 65536 padded rows (Ti ≤ 256); pick_chunk caps a
    chunk at 65536 candidates AND at a residue plane below 2^31 bytes, Mc256 ≤ (2^31 / Np256) / 256 · 256 − 256, i.e. Ti·Tj < 2^15.  The
    largest tile lists: the most row blocks (256 × 127) and the most column blocks (31 × 256, Np256 = 7936 being the widest plane that
    leaves 65536 candidates under the cap, and 32 × 255 next to it).
    Preconditions that follow from the same limits and are stated here as arithmetic:
      * accumulators: |Σ_k a·b| ≤ Np·2^14 ≤ 65536·2^14 = 2^30 < 2^31 (reached only by bytes that are all −128);
      * the epilogue's quotient |q| ≤ 2^30 / 193 < 2^23, the range of v_mad_i32_i24's 24-bit factor;
      * oz_divmod: every ticket and every divisor below 2^23; the packing: ti < 512, tj < 2048."""
    assert 65536 * 2 ** 14 <= 2 ** 30 and (2 ** 30) // 193 < 2 ** 23
    for Ti, Tj in [(256, 127), (31, 256), (32, 255)]:
        assert 256 * Ti <= 65536 and 256 * Tj <= 65536 and (256 * Ti) * (256 * Tj) < 2 ** 31
        for n in (8, 14, 16):
            blocks = assert_every_tile_once(Ti, Tj, n)
            tjg, ngi, ngj, _ = R.launch_shape(Ti, Tj, n)
            assert blocks // 8 < 2 ** 23 and max(tjg // 2, ngi, n, tjg // 8) < 2 ** 23 and Ti < 512 and Tj < 2048


def test_ticket_hook_refuses_what_the_launcher_refuses():
    L = abo._lib.lib()
    cnt = C.c_int64(0)
    for Ti, Tj, n in [(0, 1, 14), (257, 1, 14), (1, 2048, 14), (1, 1, 0), (1, 1, 17)]:
        assert L.abo_test_oz_tickets(Ti, Tj, n, None, C.byref(cnt)) == abo._lib.ABO_EINVAL
        assert "abo_test_oz_tickets" in abo._lib.last_error()
    assert L.abo_test_oz_tickets(1, 1, 14, None, None) == abo._lib.ABO_EINVAL and "null" in abo._lib.last_error()
