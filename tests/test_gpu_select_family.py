"""Direct tests of the selection family (csrc/misc.hip), piece by piece (-m gpu), through the abo_test_* hooks of the test build: the
top-k on every route of launch_topk, the survivor bookkeeping of the pruned selection (prune_compact with its scan, min_scatter, map),
the posterior epilogue's modes, and the streaming pieces (cand_gemv, downdate, grad_cov, gather_points, pick_record).

Method (tests/select_ref.py; its own checks: tests/test_select_ref_cpu.py).  The selection is held against Julia's order written from
isless in plain numpy — indices by equality, values by their bit patterns — on score families a model never produces; which route a
shape takes is asked of abo_test_topk_plan and ASSERTED, so a retuned launcher cannot silently stop covering one.  The epilogue and the
bookkeeping kernels are compared by equality with the same fp64 operations in numpy; sums against long double with a-priori bars
stated where they are used.  Every output starts as a sentinel and is checked behind its logical end; inputs carry a finite sentinel
(2⁴⁰) behind their logical width."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import (ABO_EINVAL, PRUNE_ABS, PRUNE_ABS_LOGEI, TOPK_PATH_ARGMAX as ARGMAX, TOPK_PATH_BLOCKSORT as BLOCKSORT,
                                          TOPK_PATH_SLICES as SLICES, TOPK_PATH_SMALL as SMALL, AboTestFinalizeArgs)

from tests import select_ref as R
from tests.parity_record import check

NAN = float("nan")
INF = float("inf")
eq = np.testing.assert_array_equal          # NaN == NaN at the same position
BASES = (0, 2 ** 33 + 5)
EI, UCB, PI, MEAN, LOGEI = 0, 1, 2, 3, 5


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return t.data_ptr()


def lib():
    return abo._lib.lib()


def ok(status):
    abo._lib.check(status)


def nans(*shape):
    return np.full(shape, NAN)


def eq_bits(got, want):
    """equality of fp64 arrays as bit patterns, any NaN standing for any other (−0.0 and 0.0 are told apart)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    eq(np.isnan(got), np.isnan(want))
    m = ~np.isnan(want)
    eq(R.bits(got)[m], R.bits(want)[m])


# ---- a. top-k, route by route ---------------------------------------------------------------------------------------------------------------
def route(M, k):
    out = (C.c_int64 * 6)()
    ok(lib().abo_test_topk_plan(M, k, out))
    return out[0], out


_SCORES = {}


def scores_of(fam, M):
    """one host draw, one device copy and one full reference order per (family, M), shared by every k and idx_base"""
    if (fam, M) not in _SCORES:
        s = R.scores_family(fam, M, seed=11) if M > 0 else np.array([123.0])
        _SCORES[(fam, M)] = (s, dev(s), R.sortperm_rev(s[:M], M))
    return _SCORES[(fam, M)]


def run_topk(fam, M, k, want_route):
    s, sd, order = scores_of(fam, M)
    got_route, plan = route(M, k)
    assert got_route == want_route, (M, k, list(plan))
    sel = order[:min(k, M)]
    for base in BASES:
        tv, ti = dev(np.full(k + 5, -7.0)), dev(np.full(k + 5, -7, dtype=np.int64))
        guards = C.c_int32(-1)
        ok(lib().abo_test_topk(0, ptr(sd), M, k, base, ptr(tv), ptr(ti), C.byref(guards)))
        tv, ti = host(tv), host(ti)
        assert guards.value == 1, (fam, M, k, base)                       # nothing behind topk_workspace_entries(M, k) was touched
        eq(ti[:sel.size], sel + base)
        eq(R.bits(tv[:sel.size]), R.bits(s)[sel])                         # the score's own bits: a NaN payload comes back as it went in
        eq(ti[sel.size:k], np.full(k - sel.size, -1))                     # the tail of a request longer than the batch: (NaN, −1)
        assert np.isnan(tv[sel.size:k]).all()
        eq(ti[k:], np.full(5, -7))                                        # nothing behind k
        eq(tv[k:], np.full(5, -7.0))


SMALL_MS = [0, 1, 2, 63, 1025, 16384]


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M", SMALL_MS)
def test_topk_one_workgroup(fam, M):
    """M ≤ 16384: the radix select in one workgroup wherever at most 1024 real entries are asked for; a longer request (k = M, M + 3 at
    M = 1025 and 16384) is the block-sort chain in threshold rounds.  M = 0: a scores buffer of one element, k × (NaN, −1)."""
    for k in sorted({1, 2, 129, 1024, M, M + 3} - {0}):
        run_topk(fam, M, k, SMALL if min(k, max(M, 1)) <= 1024 else BLOCKSORT)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,k", [(16385, 2), (16385, 1024), (40000, 100), (262144, 1024)])
def test_topk_slices_and_merge(fam, M, k):
    """(16385, 2): a last slice of ONE entry, shorter than k; family (b) puts the k-th entry inside a run of ties that straddles the
    slices, and the merge must keep them in index order"""
    run_topk(fam, M, k, SLICES)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M", [16385, 2048 * 9 + 1])
def test_topk_argmax_pair(fam, M):
    run_topk(fam, M, 1, ARGMAX)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,k", [(3000, 1500), (9000, 1025), (9000, 3072), (262145 + 2048, 1024)])
def test_topk_block_sort_chain(fam, M, k):
    """(3000, 1500): two rounds; (9000, 1025): a first round of four passes and a last round with kp = 1; (9000, 3072): a round
    boundary exactly at k; (264193, 1024): one pair too many for the merge of the slices"""
    run_topk(fam, M, k, BLOCKSORT)
    _, plan = route(M, k)
    assert plan[4] == -(-k // 1024)
    if (M, k) == (9000, 1025):
        assert plan[5] > 2


def test_topk_k_zero_writes_nothing():
    s, sd, _ = scores_of("a", 63)
    tv, ti = dev(np.full(4, -7.0)), dev(np.full(4, -7, dtype=np.int64))
    guards = C.c_int32(-1)
    ok(lib().abo_test_topk(0, ptr(sd), 63, 0, 0, ptr(tv), ptr(ti), C.byref(guards)))
    assert guards.value == 1
    eq(host(tv), np.full(4, -7.0))
    eq(host(ti), np.full(4, -7))


# ---- b. the pruned selection's bookkeeping -------------------------------------------------------------------------------------------------
TAU_FINITE = 0.3
PRUNE_SPECIALS = [NAN, INF, -INF, -NAN]


def _ub(M, abs_margin, rot=0):
    """uniform bounds with NaNs, ±Inf and the guard's boundary against TAU_FINITE (two ulps either side) at scattered places"""
    rng = np.random.default_rng([M, rot])
    ub = rng.uniform(-1.0, 1.0, size=M)
    sp = PRUNE_SPECIALS + list(R.guard_boundary(TAU_FINITE, abs_margin))
    sp = sp[rot % len(sp):] + sp[:rot % len(sp)]
    for i, v in enumerate(sp):
        ub[(i * 113 + 1) % M] = v                          # a batch shorter than the list keeps the last ones
    if M > 2048:                                            # a workgroup that keeps nothing and one that keeps everything
        ub[1024:2048] = -2.0
        ub[M - 1024:M - 512] = 2.0
    return ub


def _compact(ub_d, M, tau, abs_margin, sel_len):
    import torch
    tau_d = dev(np.array([tau]))
    sel = torch.full((sel_len,), -7, dtype=torch.int64, device="cuda")
    count = dev(np.array([-7, -7], dtype=np.int64))
    ok(lib().abo_test_prune_compact(0, ptr(ub_d), M, ptr(tau_d), abs_margin, ptr(sel), ptr(count)))
    return host(sel), host(count)


@pytest.mark.parametrize("M", [1, 4, 1023, 1024, 1025, 4097, 2 ** 20 + 1025])
@pytest.mark.parametrize("abs_margin", [PRUNE_ABS, PRUNE_ABS_LOGEI])
def test_prune_compact(M, abs_margin):
    """count and sel[:count] are flatnonzero of the guard in numpy, sel behind count is untouched.  2²⁰ + 1025 candidates are 1026
    workgroup counts: the scan's second trip and its carry.  tau = −Inf keeps everything, +Inf everything but NaN and ±Inf bounds
    (−Inf + Inf is NaN: kept), and on finite bounds nothing at all."""
    for rot in (range(9) if M <= 4 else (0,)):
        ub = _ub(M, abs_margin, rot)
        ub_d = dev(ub)
        for tau in (TAU_FINITE, NAN, INF, -INF):
            want = np.flatnonzero(R.prune_keep_ref(ub, tau, abs_margin))
            sel, count = _compact(ub_d, M, tau, abs_margin, M + 8)
            assert count[0] == want.size and count[1] == -7, (M, tau)
            eq(sel[:want.size], want)
            eq(sel[want.size:], np.full(M + 8 - want.size, -7))
            if tau == -INF or tau != tau:
                assert want.size == M
    fin = np.random.default_rng(M).uniform(-1.0, 1.0, size=M)
    fin_d = dev(fin)
    for tau, n_want in ((INF, 0), (5.0, 0), (-5.0, M)):                      # keep-none, keep-none by value, keep-all
        sel, count = _compact(fin_d, M, tau, abs_margin, M + 8)
        assert count[0] == n_want
        eq(sel[:n_want], np.arange(n_want))
        eq(sel[n_want:], np.full(M + 8 - n_want, -7))


def test_prune_compact_refuses_counts_its_ints_cannot_hold():
    """M = 0 and M = 2³¹ with one-element buffers: the launcher checks before it launches, nothing is read or written"""
    one, sel, count, tau = dev(np.array([1.0])), dev(np.array([-7], dtype=np.int64)), dev(np.array([-7], dtype=np.int64)), dev(np.array([0.0]))
    for M in (0, -3, 2 ** 31, 2 ** 40):
        assert lib().abo_test_prune_compact(0, ptr(one), M, ptr(tau), PRUNE_ABS, ptr(sel), ptr(count)) == ABO_EINVAL, M
    assert host(sel)[0] == -7 and host(count)[0] == -7


@pytest.mark.parametrize("n", [1, 255, 256, 1100])
def test_prune_min_scatter(n):
    """ub[sel[i]] = min(ub[sel[i]], ub2[i]): NaN on either side (and on both) gives NaN, equal values stay, entries outside sel — and
    behind the array — are untouched"""
    rng = np.random.default_rng(n)
    N = 3 * n + 7
    ub = rng.uniform(-1, 1, size=N + 3)
    sel = np.sort(rng.choice(N, size=n, replace=False)).astype(np.int64)
    ub2 = rng.uniform(-1, 1, size=n)
    ub2[::5] = ub[sel[::5]]                                 # equal
    ub2[1::7] = NAN                                         # NaN in the second level's bound
    ub[sel[2::7]] = NAN                                     # … in the first level's
    if n > 20:
        ub[sel[8]], ub2[8] = NAN, NAN
        ub[sel[9]], ub2[9] = -INF, INF
        ub[sel[10]], ub2[10] = INF, -INF
    want = ub.copy()
    a, b = ub[sel], ub2
    with np.errstate(invalid="ignore"):
        want[sel] = np.where(np.isnan(a) | np.isnan(b), NAN, np.where(b < a, b, a))
    ub_d, sel_d, ub2_d = dev(ub), dev(np.concatenate([sel, [N + 1]])), dev(np.concatenate([ub2, [-9.0]]))
    ok(lib().abo_test_prune_min_scatter(0, ptr(ub_d), ptr(sel_d), ptr(ub2_d), n))
    eq_bits(host(ub_d), want)


@pytest.mark.parametrize("k", [1, 300])
@pytest.mark.parametrize("base", BASES)
def test_prune_map(k, base):
    rng = np.random.default_rng(k)
    sel = np.sort(rng.choice(10 ** 6, size=500, replace=False)).astype(np.int64)
    ti = rng.integers(0, 500, size=k + 4).astype(np.int64)
    ti[::3] = -1
    want = ti.copy()
    m = ti[:k] >= 0
    want[:k][m] = sel[ti[:k][m]] + base                     # −1 stays, and so does everything behind k
    ti_d, sel_d = dev(ti), dev(sel)
    ok(lib().abo_test_prune_map(0, ptr(ti_d), k, ptr(sel_d), base))
    eq(host(ti_d), want)


# ---- c. the epilogue ---------------------------------------------------------------------------------------------------------------------------
J0 = 37


def _fin_case(T, Mc, seed, degenerate=False):
    """a chunk of Mc rows from global row J0 of M = J0 + Mc − 5 candidates (M ends inside the chunk); global arrays carry 4 entries
    behind M, partial / mu_in the finite sentinel in the rows behind M and in the columns behind Mc"""
    rng = np.random.default_rng([T, Mc, seed])
    M, ldp = J0 + Mc - 5, Mc + 3
    valid = M - J0
    partial = np.full((T, ldp), R.SENTINEL)
    partial[:, :valid] = rng.uniform(0.0, 0.6 / T, size=(T, valid))
    mu_in = np.full(Mc, R.SENTINEL)
    mu_in[:valid] = rng.uniform(-1.0, 1.0, size=valid)
    if degenerate:                                          # σ² = 1e-18 ≤ 1e-12 with μ above the incumbent: EI = 0, LogEI = −Inf
        partial[:, :valid:4] = 0.0
        partial[0, :valid:4] = 1.0
        mu_in[:valid:4] = 0.5
    g = lambda lo, hi: rng.uniform(lo, hi, size=M + 4)
    return dict(T=T, Mc=Mc, M=M, ldp=ldp, partial=partial, mu_in=mu_in, tail=g(-0.5, 0.5), eps=g(0.0, 1e-3), head=g(-1.0, 1.0),
                ssq=g(0.0, 0.2))


def _finalize(c, kind=-1, p0=0.0, best_y=0.0, sigma_f2=1.0, prior_grad=0.0, pc=1, point_major=0, Mpts=0, tail=False, head=False,
              score=False):
    n = c["M"] + 4
    d = dict(partial=dev(c["partial"]), mu_in=dev(c["mu_in"]), mu_out=dev(nans(n)), var_out=dev(nans(n)))
    if score:
        d["score_out"] = dev(nans(n))
    if tail:
        d["mu_tail"], d["mu_eps"] = dev(c["tail"]), dev(c["eps"])
    if head:
        d["head_g"], d["ssq_g"] = dev(c["head"]), dev(c["ssq"])
    a = AboTestFinalizeArgs(ldp=c["ldp"], j0=J0, M=c["M"], Mpts=Mpts, sigma_f2=sigma_f2, p0=p0, best_y=best_y, prior_grad=prior_grad,
                            T=c["T"], Mc=c["Mc"], kind=kind, pc=pc, point_major=point_major, **{k: ptr(v) for k, v in d.items()})
    ok(lib().abo_test_finalize(0, C.byref(a)))
    return {k: host(v) for k, v in d.items()}, d


def _fin_ref(c, sigma_f2=1.0, prior_grad=0.0, pc=1, point_major=0, Mpts=0, tail=False, head=False):
    return R.finalize_ref(c["partial"], c["mu_in"], c["M"], J0, c["Mc"], c["T"], sigma_f2, prior_grad, pc, point_major, Mpts,
                          mu_tail=c["tail"] if tail else None, mu_eps=c["eps"] if tail else None,
                          head_g=c["head"] if head else None, ssq_g=c["ssq"] if head else None, n_out=c["M"] + 4)


FIN_SHAPES = [(T, Mc) for T in (1, 3, 17) for Mc in (16, 272)]
FIN_MODES = {
    "plain": dict(),
    "point_major": dict(pc=3, point_major=1, prior_grad=0.25, sigma_f2=1.5),
    "by_outputs": dict(pc=3, point_major=0, Mpts=J0 + 7, prior_grad=0.25, sigma_f2=1.5),     # the outputs change inside the chunk
    "tail": dict(tail=True),
    "head": dict(head=True),
    "head_tail": dict(head=True, tail=True),                                                 # the fused first level as it runs
}


@pytest.mark.parametrize("T,Mc", FIN_SHAPES)
@pytest.mark.parametrize("mode", list(FIN_MODES))
def test_finalize_modes(T, Mc, mode):
    """mu_out, var_out and mu_tail equal the same additions in numpy, in the kernel's order (row blocks in turn, prior − q + 1e-18,
    head + tail, then − ε), bit for bit; rows before j0 and from M on — the chunk's last five rows — stay NaN"""
    kw = FIN_MODES[mode]
    c = _fin_case(T, Mc, seed=1)
    out, _ = _finalize(c, **kw)
    mu, var, tl = _fin_ref(c, **kw)
    eq_bits(out["mu_out"], mu)
    eq_bits(out["var_out"], var)
    if kw.get("tail"):
        eq_bits(out["mu_tail"], tl)
        eq(out["mu_eps"], c["eps"])
    assert np.isnan(out["mu_out"][:J0]).all() and np.isnan(out["mu_out"][c["M"]:]).all()
    if mode in ("point_major", "by_outputs"):                 # the prior of a gradient output landed on the rows the reference says
        gj = np.arange(J0, c["M"])
        o = gj % 3 if mode == "point_major" else gj // (J0 + 7)
        assert (o == 0).any() and (o > 0).any()


def _score(mu, var, kind, p0, best_y):
    n = mu.shape[0]
    md, vd, sd = dev(mu), dev(var), dev(nans(n + 2))
    ok(lib().abo_test_score(0, ptr(md), ptr(vd), ptr(sd), n, kind, p0, best_y))
    s = host(sd)
    assert np.isnan(s[n:]).all()
    return s[:n]


SCORE_KINDS = [(EI, 0.01, 0.1), (UCB, 2.0, 0.0), (PI, 0.01, 0.1), (MEAN, 0.0, 0.0), (LOGEI, 0.01, 0.1)]


@pytest.mark.parametrize("T,Mc", [(3, 16), (17, 272)])
@pytest.mark.parametrize("kind,p0,best_y", SCORE_KINDS)
def test_finalize_score_is_the_plain_scoring_kernel(T, Mc, kind, p0, best_y):
    """score_out equals launch_score on the epilogue's own (μ, σ²), bit for bit, rows of degenerate variance included"""
    c = _fin_case(T, Mc, seed=2, degenerate=True)
    out, _ = _finalize(c, kind=kind, p0=p0, best_y=best_y, score=True)
    lo, hi = J0, c["M"]
    want = nans(c["M"] + 4)
    want[lo:hi] = _score(out["mu_out"][lo:hi], out["var_out"][lo:hi], kind, p0, best_y)
    eq_bits(out["score_out"], want)
    if kind == LOGEI:
        assert np.isneginf(want[lo:hi:4]).all()
    if kind == EI:
        assert (want[lo:hi:4] == 0.0).all() and (want[lo + 1:hi:4] > 1e-6).all()


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("kind,p0,best_y", [(EI, 0.01, 0.1), (UCB, 2.0, 0.0), (LOGEI, 0.01, 0.1)])
def test_finalize_stores_the_guarded_bound(head, kind, p0, best_y):
    """bound mode (mu_tail given): μ_out is μ̃ − ε, and the stored score is sc + |sc|·2⁻³⁰ + abs recomputed in numpy from the unguarded
    score of the plain scoring kernel at (μ̃ − ε, σ²).  The scores are in the normal range, where the product by 2⁻³⁰ is exact (an fma
    changes nothing); LogEI's −Inf of the degenerate rows stays −Inf (−Inf + Inf would be NaN, and NaN ranks first)."""
    c = _fin_case(3, 272, seed=3, degenerate=True)
    out, _ = _finalize(c, kind=kind, p0=p0, best_y=best_y, score=True, tail=True, head=head)
    mu, var, tl = _fin_ref(c, tail=True, head=head)
    eq_bits(out["mu_out"], mu)
    eq_bits(out["var_out"], var)
    eq_bits(out["mu_tail"], tl)
    lo, hi = J0, c["M"]
    sc = _score(out["mu_out"][lo:hi], out["var_out"][lo:hi], kind, p0, best_y)
    nz = sc[np.isfinite(sc) & (sc != 0.0)]
    assert nz.size > 100 and np.abs(nz).min() > 2.0 ** -900           # normal, and so is its 2⁻³⁰-th part
    want = nans(c["M"] + 4)
    want[lo:hi] = R.guarded(sc, PRUNE_ABS_LOGEI if kind == LOGEI else PRUNE_ABS)
    eq_bits(out["score_out"], want)
    assert (want[lo:hi][np.isfinite(sc)] >= sc[np.isfinite(sc)]).all()
    if kind == LOGEI and not head:
        assert np.isneginf(sc).any() and np.isneginf(want[lo:hi][np.isneginf(sc)]).all()


# ---- d. streaming pieces ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 16, 19])
@pytest.mark.parametrize("n", [1, 2, 127, 130, 1001])
def test_cand_gemv(M, n):
    """c[j] = Σ_{k<n} Kzx[j][k]·v[k] against a long double dot product.  A lane takes the pairs lane, lane + 64, … — elements 128 apart,
    two fused multiply-adds a trip — and the 64 lanes meet in a six-level tree.  The bar is γ_{⌈n/128⌉+8}·Σ|Kzx·v|: one rounding a trip
    of a lane's chain, the six tree additions, two to spare.  (Counting both fmas of a trip the worst case is γ_{2⌈n/128⌉+6}, the same
    up to n = 256 and 22 against 16 roundings at n = 1001; the tighter figure is the one held.)  Columns ≥ n of Kzx and v hold 2⁴⁰: the
    odd end of the last pair meets v = 0, nothing further right is read; rows M mod 4 ≠ 0 of the last wave are not written."""
    rng = np.random.default_rng([M, n])
    ld = n + 1 + ((n + 1) & 1) + 2
    K = np.full((M, ld), R.SENTINEL)
    K[:, :n] = rng.standard_normal((M, n))
    v = np.full(ld, R.SENTINEL)
    v[:n] = rng.standard_normal(n)
    Kd, vd, cd = dev(K), dev(v), dev(nans(M + 3))
    ok(lib().abo_test_cand_gemv(0, ptr(Kd), ld, ptr(vd), n, M, ptr(cd)))
    c = host(cd)
    assert np.isnan(c[M:]).all()
    prod = K[:, :n].astype(R.LD) * v[:n].astype(R.LD)
    ref, mag = prod.sum(axis=1), np.abs(prod).sum(axis=1).astype(np.float64)
    err = np.abs((c[:M].astype(R.LD) - ref).astype(np.float64))
    bar = R.gamma(math.ceil(n / 128) + 8) * mag
    print(f"cand_gemv M = {M}, n = {n}: max err / bar = {np.max(err / bar):.3f}")
    assert (err <= bar).all()


@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
def test_downdate(M):
    """μ' = fma(c, β, μ) — long double, rounded once, on operands whose product needs 60 bits: a multiply followed by an add gives
    another result on a good part of them — and σ²' = σ² − c·c/s2 in fp64 in that order; nothing behind M"""
    c, beta, mu, var, s2 = R.downdate_operands(M, seed=M)
    pad = lambda a: np.concatenate([a, [NAN, NAN]])
    md, vd, cd = dev(pad(mu)), dev(pad(var)), dev(pad(c))
    ok(lib().abo_test_downdate(0, ptr(md), ptr(vd), ptr(cd), M, beta, s2))
    eq_bits(host(md), pad(R.fma_ref(c, beta, mu)))
    eq_bits(host(vd), pad(var - c * c / s2))


@pytest.mark.parametrize("p", [2, 33, 129])
@pytest.mark.parametrize("R_", [1, 63, 64, 200])
def test_grad_cov(p, R_):
    """cov_out[q][q'] = prior − Σ_{i<R} V_q[i]·V_q'[i] per point (p = 129: 134 KB of dynamic LDS, the raised limit).  Symmetric bit for
    bit; against long double within γ_{⌈R/64⌉+7}·Σ|v₁v₂| + u·|C| (a lane's ⌈R/64⌉ fmas, six tree additions, one to spare, and the final
    subtraction's own rounding); mu_out by equality; the GradientNormUCB score against the formula in long double on the hook's own
    (m, C), within the bar tests/select_ref.py: gradnorm_ref derives from the operation count of gradnorm_moments."""
    rng = np.random.default_rng([p, R_])
    npts, pt0, ldv = 3, 2, R_ + 3
    prior0, prior_g, beta = 1.0, 2.0, 1.7
    V = np.full((npts * p, ldv), R.SENTINEL)
    V[:, :R_] = rng.uniform(-1.0, 1.0, size=(npts * p, R_)) / math.sqrt(R_)
    mu_rows = rng.uniform(-1.0, 1.0, size=npts * p)
    tot = pt0 + npts + 1
    Vd, md = dev(V), dev(mu_rows)
    cov, mu, sc = dev(nans(tot, p, p)), dev(nans(tot, p)), dev(nans(tot))
    ok(lib().abo_test_grad_cov(0, ptr(Vd), ptr(md), ldv, R_, p, pt0, prior0, prior_g, beta, ptr(cov), ptr(mu), ptr(sc), npts))
    cov, mu, sc = host(cov), host(mu), host(sc)
    live = slice(pt0, pt0 + npts)
    for a in (cov, mu, sc):                                   # nothing in front of pt0, nothing behind the last point
        assert np.isnan(a[:pt0]).all() and np.isnan(a[pt0 + npts:]).all() and np.isfinite(a[live]).all()
    eq(mu[live], mu_rows.reshape(npts, p))
    eq(R.bits(cov[live]), R.bits(np.swapaxes(cov[live], 1, 2)))
    case = f"select/grad_cov_p{p}_R{R_}"
    worst_c, worst_s = 0.0, 0.0
    for j in range(npts):
        Vj = V[j * p:(j + 1) * p, :R_].astype(R.LD)
        prior = np.zeros((p, p))
        prior[np.arange(p), np.arange(p)] = np.float64(prior_g) + 1e-18
        prior[0, 0] = np.float64(prior0) + 1e-18
        ref = prior.astype(R.LD) - Vj @ Vj.T
        mag = (np.abs(Vj) @ np.abs(Vj).T).astype(np.float64)
        err = np.abs((cov[pt0 + j].astype(R.LD) - ref).astype(np.float64))
        bar = R.gamma(math.ceil(R_ / 64) + 7) * mag + R.U * np.abs(cov[pt0 + j])
        assert (err <= bar).all(), (j, float(np.max(err / bar)))
        worst_c = max(worst_c, float(np.max(err / bar)))
        want, sbar = R.gradnorm_ref(mu[pt0 + j], cov[pt0 + j], beta)
        serr = abs(sc[pt0 + j] - want)
        print(f"{case} point {j}: score {sc[pt0 + j]:.6e}, |err| {serr:.3e}, bar {sbar:.3e}")
        assert serr <= sbar
        worst_s = max(worst_s, serr / sbar)
    check(case, "cov_err_over_bar", worst_c, 1.0, tighten=False)
    check(case, "score_err_over_bar", worst_s, 1.0, tighten=False)
    # without the optional outputs: the score alone is the same
    sc2 = dev(nans(tot))
    ok(lib().abo_test_grad_cov(0, ptr(Vd), ptr(md), ldv, R_, p, pt0, prior0, prior_g, beta, None, None, ptr(sc2), npts))
    eq(host(sc2), sc)


@pytest.mark.parametrize("d", [1, 3, 64])
@pytest.mark.parametrize("base", BASES)
def test_gather_points_and_pick_record(d, base):
    """negative indices give zeros, idx_base is taken off; nothing behind k·d / behind 3 + d"""
    rng = np.random.default_rng(d)
    nZ, k = 50, 9
    Z, mu = rng.standard_normal((nZ, d)), rng.standard_normal(nZ)
    loc = rng.integers(0, nZ, size=k)
    idx = (loc + base).astype(np.int64)
    idx[[2, 5]] = -1
    Zd, mud, idx_d, out = dev(Z), dev(mu), dev(idx), dev(nans(k * d + 3))
    ok(lib().abo_test_gather_points(0, ptr(Zd), ptr(idx_d), base, k, d, ptr(out)))
    want = nans(k * d + 3)
    want[:k * d] = np.where((idx >= 0)[:, None], Z[loc], 0.0).reshape(-1)
    eq_bits(host(out), want)
    for e in (0, 2):                                          # a real pick and an empty one
        tv, ti, rec = dev(np.array([0.625])), dev(idx[e:e + 1]), dev(nans(3 + d + 2))
        ok(lib().abo_test_pick_record(0, ptr(tv), ptr(ti), base, ptr(Zd), ptr(mud), d, ptr(rec)))
        want = nans(3 + d + 2)
        want[:3 + d] = np.concatenate([[0.625, float(idx[e]), mu[loc[e]]], Z[loc[e]]]) if idx[e] >= 0 else \
            np.concatenate([[0.625, -1.0, 0.0], np.zeros(d)])
        eq_bits(host(rec), want)


# ---- e. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_hooks_refuse_what_the_launchers_cannot_take():
    """null pointers and impossible shapes come back as ABO_EINVAL with no launch: every output still holds its sentinel"""
    z = dev(np.full(8, -7.0))
    zi = dev(np.full(8, -7, dtype=np.int64))
    p, pi = ptr(z), ptr(zi)
    L = lib()
    g = C.c_int32(-1)
    assert L.abo_test_topk(0, None, 4, 1, 0, p, pi, C.byref(g)) == ABO_EINVAL
    assert L.abo_test_topk(0, p, 4, 1, 0, p, pi, None) == ABO_EINVAL
    assert L.abo_test_topk(0, p, -1, 1, 0, p, pi, C.byref(g)) == ABO_EINVAL
    assert L.abo_test_topk(0, p, 4, -1, 0, p, pi, C.byref(g)) == ABO_EINVAL
    assert g.value == -1
    assert L.abo_test_prune_compact(0, None, 4, p, 0.0, pi, pi) == ABO_EINVAL
    assert L.abo_test_prune_compact(0, p, 4, None, 0.0, pi, pi) == ABO_EINVAL
    assert L.abo_test_prune_min_scatter(0, p, None, p, 1) == ABO_EINVAL
    assert L.abo_test_prune_min_scatter(0, p, pi, p, -1) == ABO_EINVAL
    assert L.abo_test_prune_map(0, None, 1, pi, 0) == ABO_EINVAL
    assert L.abo_test_prune_map(0, pi, -1, pi, 0) == ABO_EINVAL
    assert L.abo_test_finalize(0, None) == ABO_EINVAL
    okay = dict(partial=p, mu_in=p, mu_out=p, var_out=p, ldp=4, j0=0, M=4, T=1, Mc=4, kind=-1, pc=1, sigma_f2=1.0)
    for bad in (dict(partial=None), dict(mu_in=None), dict(mu_tail=p), dict(T=-1), dict(Mc=-1), dict(ldp=3), dict(pc=0), dict(j0=-1),
                dict(pc=2, point_major=0, Mpts=0)):
        a = AboTestFinalizeArgs(**dict(okay, **bad))
        assert L.abo_test_finalize(0, C.byref(a)) == ABO_EINVAL, bad
    assert L.abo_test_cand_gemv(0, None, 4, p, 2, 1, p) == ABO_EINVAL
    assert L.abo_test_cand_gemv(0, p, 5, p, 2, 1, p) == ABO_EINVAL                 # odd ld
    assert L.abo_test_cand_gemv(0, p, 2, p, 2, 1, p) == ABO_EINVAL                 # ld < n + 1
    assert L.abo_test_cand_gemv(0, p, 4, p + 8, 2, 1, p) == ABO_EINVAL             # v not 16-byte aligned
    assert L.abo_test_downdate(0, p, None, p, 1, 1.0, 1.0) == ABO_EINVAL
    assert L.abo_test_downdate(0, p, p, p, -1, 1.0, 1.0) == ABO_EINVAL
    assert L.abo_test_grad_cov(0, None, p, 4, 2, 2, 0, 1.0, 1.0, 1.0, p, p, p, 1) == ABO_EINVAL
    assert L.abo_test_grad_cov(0, p, p, 1, 2, 2, 0, 1.0, 1.0, 1.0, p, p, p, 1) == ABO_EINVAL      # ldv < R
    assert L.abo_test_grad_cov(0, p, p, 4, 2, 0, 0, 1.0, 1.0, 1.0, p, p, p, 1) == ABO_EINVAL      # p < 1
    assert L.abo_test_grad_cov(0, p, p, 4, 2, 143, 0, 1.0, 1.0, 1.0, p, p, p, 1) == ABO_EINVAL    # C and m beyond a workgroup's LDS: the launcher's refusal
    assert L.abo_test_gather_points(0, p, None, 0, 1, 1, p) == ABO_EINVAL
    assert L.abo_test_gather_points(0, p, pi, 0, 1, 0, p) == ABO_EINVAL
    assert L.abo_test_pick_record(0, p, pi, 0, p, None, 1, p) == ABO_EINVAL
    assert L.abo_test_pick_record(0, p, pi, 0, p, p, 0, p) == ABO_EINVAL
    assert L.abo_test_score(0, p, p, None, 1, 0, 0.0, 0.0) == ABO_EINVAL
    assert L.abo_test_score(0, p, p, p, 1, 4, 0.0, 0.0) == ABO_EINVAL              # GRADNORM_UCB is no epilogue on (μ, σ²)
    assert L.abo_test_score(0, p, p, p, -1, 0, 0.0, 0.0) == ABO_EINVAL
    eq(host(z), np.full(8, -7.0))
    eq(host(zi), np.full(8, -7))
