"""GPU tests (-m gpu) of sample paths that follow the model through appends (abo_paths_append, _attach, _top, _values;
include/abo_hip.h).

The reference is the dense NumPy/SciPy restatement in tests/test_thompson_append_cpu.py, neither route touching the device:
`restate_scratch` (the header's four formulas on the N + k points, `eps` extended by the ε* columns) and `restate_incremental`
(the append formulas applied k times).  Bar of a case — measured, not fixed: δ_case = their largest disagreement over all paths and
test candidates in units of sqrt(σ_f²); the library must be within min(1e-6, max(100·δ_case, 1e-12)) of the from-scratch route
(100 × is parity_record.MARGIN: the device sums in another order than either).  Every comparison goes through
tests.parity_record.check under thompson_append/*, so the achieved error is recorded."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import thompson
from oracle import gp_oracle as O

from tests.parity_record import MARGIN, check
from tests.test_gpu_parity import FAMS, make_model
from tests.test_thompson_append_cpu import delta_of, restate_incremental, restate_scratch

HARD = 1e-6


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def make(family, d, N, k, S, R, noise, ell, mean_c=0.0, sf2=1.4, seed=0, spread=False, n_max=None):
    """(rng, X (N + k, d), y, hp, base with eps (S, N + k), model on the first N points with room for the appends)"""
    rng = np.random.default_rng(7000 + seed)
    if spread:                                              # well-separated points: a jittered lattice
        side = int(math.ceil((N + k) ** (1.0 / d)))
        grid = np.stack(np.meshgrid(*[np.arange(side)] * d, indexing="ij"), axis=-1).reshape(-1, d)[:N + k]
        X = (grid + 0.5 + 0.1 * (rng.random((N + k, d)) - 0.5)) / side
        X = X[rng.permutation(N + k)]
    else:
        X = rng.random((N + k, d))
    y = np.sin(3.0 * X.sum(axis=1) / math.sqrt(d)) + 0.3 * np.cos(5.0 * X[:, 0]) + 0.05 * rng.standard_normal(N + k)
    hp = (family, ell, sf2, noise, mean_c)
    base = thompson.draw_base(FAMS[family](), S, R, N + k, d, rng)
    model = abo.update(make_model(family, ell, sf2, noise, mean_c, n_max=n_max or (N + k + 64)), X[:N], y[:N])
    return rng, X, y, hp, base, model


def sub_base(base, n):
    return base[0], base[1], base[2], np.ascontiguousarray(base[3][:, :n])


def case_bar(hp, X, y, base, Z, k):
    g = restate_scratch(hp, X, y, base, Z)
    g_inc, _ = restate_incremental(hp, X, y, base, Z, k)
    delta = delta_of(hp, g, g_inc)
    assert MARGIN * delta <= HARD, f"the case is ill-conditioned for the restatement itself (delta {delta:.3e}): replace it"
    return g, delta, min(HARD, max(MARGIN * delta, 1e-12))


#        name                 family d   N     S   R     noise  ell   spread
CASES = [("se_d2_n37_noise0",  0,     2,  37,   16, 256,  0.0,   0.12, True),
         ("m52_d2_n37",        1,     2,  37,   17, 256,  1e-3,  0.3,  False),
         ("se_d8_n300",        0,     8,  300,  16, 512,  1e-3,  1.0,  False),     # N a multiple of 4
         ("m52_d8_n300",       1,     8,  300,  33, 512,  1e-4,  0.9,  False),
         ("m52_d16_n2048",     1,     16, 2046, 64, 1024, 1e-3,  1.5,  False),     # 2046 + 5 crosses 2048 = 16·128
         ("se_d16_n2048",      0,     16, 2048, 64, 512,  1e-2,  1.6,  False),
         ("m52_d16_n37",       1,     16, 37,   16, 64,   1e-3,  1.4,  False)]


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("name,family,d,N,S,R,noise,ell,spread", CASES, ids=[c[0] for c in CASES])
def test_advanced_paths_equal_fresh_paths(name, family, d, N, S, R, noise, ell, spread, k):
    rng, X, y, hp, base, model = make(family, d, N, k, S, R, noise, ell, seed=N + d + k, spread=spread)
    Z = rng.random((300, d))
    g, delta, bar = case_bar(hp, X, y, base, Z, k)
    paths = abo.SamplePaths(model, *sub_base(base, N))
    m = model
    for j in range(k):
        m = abo.append(m, X[N + j], float(y[N + j]))
        paths.append(m, base[3][:, N + j])
    assert np.array_equal(paths.eps, base[3]) and paths.stats()["N"] == N + k and paths.append_stats()["appends"] == k
    assert paths.append_stats()["column_from_chain"] == -1 and paths.append_stats()["model_ms"] > 0.0
    vals = paths(Z)
    sq = math.sqrt(hp[2])
    err = float(np.max(np.abs(vals - g))) / sq
    fresh = abo.SamplePaths(m, *base)(Z)
    err2 = float(np.max(np.abs(vals - fresh))) / sq
    print(f"{name} k={k}: delta_case {delta:.3e}  bar {bar:.3e}  achieved vs restatement {err:.3e}  vs abo_paths_create {err2:.3e}")
    check(f"thompson_append/{name}_k{k}", "values_over_sqrt_sf2", err, bar)
    check(f"thompson_append/{name}_k{k}", "against_fresh_paths_over_sqrt_sf2", err2, 2.0 * bar)
    assert np.array_equal(bits(paths(Z)), bits(vals))


def run_resident(seed, from_chain, M=5003, k=5, family=1, d=4, N=200, S=17, R=256, noise=1e-3, ell=0.6):
    """attach, then k × (abo_append → abo_cand_downdate → abo_paths_append); the appended points are picks of a preceding abo_cand_qei
    batch (from_chain) or arbitrary.  Returns everything the checks need, step by step."""
    rng, X, y, hp, base, model = make(family, d, N, k, S, R, noise, ell, seed=seed, n_max=1024)
    Z = rng.random((M, d))
    cands = abo.ResidentCandidates(model, Z)
    if from_chain:
        # a batch of q picks leaves the chain c_1 … c_{q−1} with the set (the last pick conditions nothing): k + 1 picks serve k appends
        Xq, idx, _, _ = cands.qei(k + 1, 0.01, float(y[:N].min()), distinct=True)
        Xq = Xq[:k]
        X[N:] = Xq
        y[N:] = np.sin(3.0 * Xq.sum(axis=1) / math.sqrt(d)) + 0.3 * np.cos(5.0 * Xq[:, 0])
    paths = abo.SamplePaths(model, *sub_base(base, N))
    paths.attach(cands)
    steps, m = [], model
    v0 = paths.values()
    assert np.array_equal(bits(v0), bits(paths(cands)))                  # attach keeps what the evaluation pass gives
    for j in range(k):
        m = abo.append(m, X[N + j], float(y[N + j]))
        cands.downdate(m)
        tm = timings_of(m)
        paths.append(m, base[3][:, N + j])
        st = paths.append_stats()
        vals = paths.values()
        tv1, ti1 = paths.top(1)
        tv7, ti7 = paths.top(7, idx_base=100)
        steps.append(dict(vals=vals, tv1=tv1, ti1=ti1, tv7=tv7, ti7=ti7, st=st, tm=tm))
    return dict(hp=hp, X=X, y=y, base=base, Z=Z, N=N, k=k, steps=steps, paths=paths, cands=cands, model=m)


def timings_of(model):
    t = abo._lib.AboTimings()
    abo._lib.check(abo._lib.lib().abo_get_timings(model._require(), C.byref(t)))
    return t.as_dict()


@pytest.mark.parametrize("from_chain", [True, False], ids=["chain", "pass"])
def test_resident_values_and_picks_follow_the_model(from_chain):
    r = run_resident(31 + int(from_chain), from_chain)
    hp, X, y, base, Z, N = r["hp"], r["X"], r["y"], r["base"], r["Z"], r["N"]
    S, M = base[2].shape[0], Z.shape[0]
    for j, stp in enumerate(r["steps"]):
        n = N + j + 1
        g, delta, bar = case_bar(hp, X[:n], y[:n], sub_base(base, n), Z, j + 1)
        vals = stp["vals"]
        err = float(np.max(np.abs(vals - g))) / math.sqrt(hp[2])
        print(f"resident {'chain' if from_chain else 'pass'} step {j + 1}: delta {delta:.3e} bar {bar:.3e} achieved {err:.3e} stats {stp['st']}")
        check(f"thompson_append/resident_{'chain' if from_chain else 'pass'}_step{j + 1}", "values_over_sqrt_sf2", err, bar)
        assert stp["st"]["column_from_chain"] == (1 if from_chain else 0)
        assert stp["tm"]["downdate_from_chain"] == (1 if from_chain else 0)
        assert stp["st"]["resident_bytes"] == 16.0 * S * M + 8.0 * M and stp["st"]["resident_ms"] > 0.0
        assert stp["tv1"].shape == (S, 1) and stp["ti1"].shape == (S, 1)
        assert np.array_equal(stp["ti1"][:, 0], np.argmin(vals, axis=1))                       # the FIRST arg-min of those very values
        assert np.array_equal(bits(stp["tv1"][:, 0]), bits(vals[np.arange(S), stp["ti1"][:, 0]]))
        order = np.argsort(vals, axis=1, kind="stable")[:, :7]
        assert np.array_equal(stp["ti7"] - 100, order)
        assert np.array_equal(bits(stp["tv7"]), bits(np.take_along_axis(vals, order, axis=1)))
    # the object itself followed too: its evaluation pass on the appended model agrees with the resident values within the bar
    ev = r["paths"](r["cands"])
    check(f"thompson_append/resident_{'chain' if from_chain else 'pass'}_eval", "resident_against_eval_over_sqrt_sf2",
          float(np.max(np.abs(ev - r["steps"][-1]["vals"]))) / math.sqrt(hp[2]), 2.0 * bar)


@pytest.mark.parametrize("kzx_gib", ["64", "0"], ids=["resident", "recomputing"])
def test_the_recomputed_column_serves_a_set_whose_down_date_was_not_the_last_writer(monkeypatch, kzx_gib):
    """two sets down-dated with the same appended model: each finds its own column; a set that was refreshed to the appended model
    instead of down-dated has no column in place and gets it recomputed (column_from_chain == 2) — never a stale one.  Under both
    budgets of the resident K_ZX: with it the column is one product over K_ZX, without it the kernel values are evaluated again"""
    monkeypatch.setenv("ABO_CAND_KZX_GIB", kzx_gib)
    rng, X, y, hp, base, model = make(1, 3, 120, 2, 16, 128, 1e-3, 0.5, seed=77, n_max=512)
    Z = rng.random((1500, 3))
    cands = abo.ResidentCandidates(model, Z)
    paths = abo.SamplePaths(model, *sub_base(base, 120))
    paths.attach(cands)
    m1 = abo.append(model, X[120], float(y[120]))
    cands.downdate(m1)
    paths.append(m1, base[3][:, 120])
    assert paths.append_stats()["column_from_chain"] == 0
    m2 = abo.append(m1, X[121], float(y[121]))
    cands.refresh(m2)                                         # in sync with m2, but cdot still holds the column of m1's append
    paths.append(m2, base[3][:, 121])
    assert paths.append_stats()["column_from_chain"] == 2
    g, delta, bar = case_bar(hp, X, y, base, Z, 2)
    check("thompson_append/recomputed_column", "values_over_sqrt_sf2", float(np.max(np.abs(paths.values() - g))) / math.sqrt(hp[2]), bar)


def test_exclusions_short_sets_and_a_set_of_one():
    rng, X, y, hp, base, model = make(1, 3, 90, 2, 16, 128, 1e-3, 0.5, seed=5, n_max=256)
    Z = rng.random((700, 3))
    cands = abo.ResidentCandidates(model, Z)
    paths = abo.SamplePaths(model, *sub_base(base, 90))
    paths.attach(cands)
    tv, ti = paths.top(1)
    gone = sorted(set(int(j) for j in ti[:, 0]))
    for j in gone:
        cands.exclude(j)                                      # AFTER attach: exclusions are read when the selection runs
    tv2, ti2 = paths.top(1)
    vals = paths.values()
    assert np.all(np.isposinf(vals[:, gone])) and not np.isin(ti2, gone).any()
    assert np.array_equal(ti2[:, 0], np.argmin(vals, axis=1)) and np.array_equal(bits(tv2[:, 0]), bits(vals[np.arange(16), ti2[:, 0]]))
    m1 = abo.append(model, X[90], float(y[90]))
    cands.downdate(m1)
    paths.append(m1, base[3][:, 90])
    tv3, ti3 = paths.top(1)
    vals = paths.values()
    assert np.all(np.isposinf(vals[:, gone])) and not np.isin(ti3, gone).any()
    assert np.array_equal(ti3[:, 0], np.argmin(vals, axis=1))
    _, ti9 = paths.top(9)
    assert not np.isin(ti9, gone).any()
    # M < k: the (NaN, −1) tail; a set of one candidate
    for Msmall in (3, 1):
        c2 = abo.ResidentCandidates(model, Z[:Msmall])
        p2 = abo.SamplePaths(model, *sub_base(base, 90))
        p2.attach(c2)
        tv, ti = p2.top(5)
        assert np.all(ti[:, Msmall:] == -1) and np.all(np.isnan(tv[:, Msmall:])) and np.all(ti[:, :Msmall] >= 0)
        tv1, ti1 = p2.top(1)
        v = p2.values()
        assert v.shape == (16, Msmall) and np.array_equal(ti1[:, 0], np.argmin(v, axis=1))
        c2.downdate(m1)
        p2.append(m1, base[3][:, 90])
        tv1, ti1 = p2.top(1)
        assert np.array_equal(ti1[:, 0], np.argmin(p2.values(), axis=1))
        if Msmall == 1:
            c2.exclude(0)
            tv1, ti1 = p2.top(1)
            assert np.all(ti1 == 0) and np.all(np.isposinf(tv1))      # every candidate excluded: the first of them, at +Inf
        p2.detach()


def test_the_five_step_sequence_is_deterministic():
    a, b = run_resident(41, True), run_resident(41, True)
    for sa, sb in zip(a["steps"], b["steps"]):
        for key in ("vals", "tv1", "tv7"):
            assert np.array_equal(bits(sa[key]), bits(sb[key])), key
        assert np.array_equal(sa["ti1"], sb["ti1"]) and np.array_equal(sa["ti7"], sb["ti7"])


def test_refusals_leave_the_object_untouched():
    rng, X, y, hp, base, model = make(1, 2, 61, 3, 16, 128, 1e-3, 0.4, seed=6, n_max=128)
    L, EINVAL = abo._lib.lib(), abo._lib.ABO_EINVAL
    Z = rng.random((400, 2))
    paths = abo.SamplePaths(model, *sub_base(base, 61))
    before = paths(Z)
    e = np.ascontiguousarray(base[3][:, 61])
    m1 = abo.append(model, X[61], float(y[61]))
    m2 = abo.append(m1, X[62], float(y[62]))

    def refused(handle, eps=e, match=None):
        rc = L.abo_paths_append(paths._h.ptr, handle, eps.ctypes.data if eps is not None else None, abo._lib.HOST)
        assert rc == EINVAL, (rc, abo._lib.last_error())
        if match:
            assert match in abo._lib.last_error(), abo._lib.last_error()
        assert np.array_equal(bits(paths(Z)), bits(before))
    refused(m2._require(), match="ONE append ahead")                                 # two appends ahead
    refit = abo.update(make_model(1, 0.4, 1.4, 1e-3, 0.0, n_max=128), X[:62], y[:62])
    refused(refit._require(), match="lineage")                                       # a refit of the same data
    other = abo.append(abo.update(make_model(1, 0.4, 1.4, 1e-3, 0.0, n_max=128), X[:61], y[:61]), X[61], float(y[61]))
    refused(other._require(), match="lineage")                                       # another lineage
    gm = abo.HipGradientGP(abo.SqExponentialKernel(), 3, 1e-3)
    Xg = rng.random((6, 2))
    gm = abo.update(gm, Xg, [[math.sin(x[0]), math.cos(x[0]), 0.0] for x in Xg])
    refused(gm._require(), match="gradient-enhanced")
    refused(None, match="null")
    refused(m1._require(), eps=None, match="null")
    bad = e.copy()
    bad[3] = np.inf
    refused(m1._require(), eps=bad, match="finite")
    # a full model whose append falls back to a refit is a refit in disguise
    small = abo.update(make_model(1, 0.4, 1.4, 1e-3, 0.0, n_max=128), X[:61], y[:61])
    full = small
    for _ in range(128 - 61):                                                          # fill the capacity (128 rows)
        full = abo.append(full, rng.random(2), 0.1)
    pf = abo.SamplePaths(full, *thompson.draw_base(FAMS[1](), 16, 64, 128, 2, rng))
    vf = pf(Z)
    over = abo.append(full, rng.random(2), 0.2)
    assert L.abo_paths_append(pf._h.ptr, over._require(), e.ctypes.data, abo._lib.HOST) == EINVAL
    assert np.array_equal(bits(pf(Z)), bits(vf))
    # attached set: not down-dated to the new model; a set of another dimension is refused at attach
    cands = abo.ResidentCandidates(model, Z)
    with pytest.raises(abo.DimensionMismatch):
        paths.attach(abo.ResidentCandidates(abo.update(make_model(1, 0.4, 1.4, 1e-3), rng.random((20, 3)), rng.random(20)), rng.random((50, 3))))
    paths.attach(cands)
    v0 = paths.values()
    refused(m1._require(), match="abo_cand_downdate")
    assert np.array_equal(bits(paths.values()), bits(v0))
    cands.downdate(m1)
    paths.append(m1, e)                                                               # … and the accepted step goes through
    assert not np.array_equal(bits(paths.values()), bits(v0))
    with pytest.raises(ValueError):
        paths.append(m1, e)                                                           # the same model again: not one append ahead


def test_lifetime_the_object_retains_the_appended_model_and_releases_the_old_one():
    rng, X, y, hp, base, model = make(1, 2, 61, 1, 16, 128, 1e-3, 0.4, seed=9, n_max=128)
    Z = rng.random((300, 2))
    g, delta, bar = case_bar(hp, X, y, base, Z, 1)
    paths = abo.SamplePaths(model, *sub_base(base, 61))
    m1 = abo.append(model, X[61], float(y[61]))
    paths.append(m1, base[3][:, 61])
    want = paths(Z)
    paths.model = None
    del model, m1                                             # the caller's references to BOTH models go
    gc.collect()
    got = paths(Z)
    assert np.array_equal(bits(got), bits(want))
    check("thompson_append/lifetime", "values_over_sqrt_sf2", float(np.max(np.abs(got - g))) / math.sqrt(hp[2]), bar)


def test_config5_shape_three_appends_against_the_restatement():
    """N = 16 384, d = 16, M = 131 072, S = 64, R = 1024, 3 appends: values on a subsample of 1 024 candidates and ALL top-1 picks
    against the from-scratch restatement on an independent CPU factorisation of the N + 3 points.  A pick may differ from the
    restatement's where two candidates lie within the bar of each other: every differing pick's restated value must be within 2 × bar
    of the restated minimum, and at most S/8 paths may differ."""
    N, d, M, S, R, k = 16384, 16, 131072, 64, 1024, 3
    rng, X, y, hp, base, model = make(1, d, N, k, S, R, 1e-3, 1.5, seed=16, n_max=N + 128)
    Z = rng.random((M, d))
    cands = abo.ResidentCandidates(model, Z)
    paths = abo.SamplePaths(model, *sub_base(base, N))
    paths.attach(cands)
    m = model
    for j in range(k):
        m = abo.append(m, X[N + j], float(y[N + j]))
        cands.downdate(m)
        paths.append(m, base[3][:, N + j])
        print("config-5 shape step", j + 1, paths.append_stats())
    tv, ti = paths.top(1)
    sub = np.arange(0, M, M // 1024)[:1024]
    vals = paths.values()
    g = restate_scratch(hp, X, y, base, Z)
    g_inc, _ = restate_incremental(hp, X, y, base, Z[sub], k)
    delta = delta_of(hp, g[:, sub], g_inc)
    assert MARGIN * delta <= HARD
    bar = min(HARD, max(MARGIN * delta, 1e-12))
    sq = math.sqrt(hp[2])
    err = float(np.max(np.abs(vals[:, sub] - g[:, sub]))) / sq
    err_all = float(np.max(np.abs(vals - g))) / sq
    print(f"config-5 shape: delta_case {delta:.3e}  bar {bar:.3e}  achieved on the subsample {err:.3e}  on all candidates {err_all:.3e}")
    check("thompson_append/config5_shape", "values_over_sqrt_sf2", err, bar)
    assert np.array_equal(ti[:, 0], np.argmin(vals, axis=1)) and np.array_equal(bits(tv[:, 0]), bits(vals[np.arange(S), ti[:, 0]]))
    want = np.argmin(g, axis=1)
    differ = [s for s in range(S) if ti[s, 0] != want[s]]
    for s in differ:
        assert g[s, ti[s, 0]] - g[s, want[s]] <= 2.0 * bar * sq, (s, g[s, ti[s, 0]] - g[s, want[s]])
    check("thompson_append/config5_shape", "differing_picks_fraction", len(differ) / S, 1.0 / 8.0, tighten=False)
