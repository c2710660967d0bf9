"""GPU tests (-m gpu) of Thompson sampling: pathwise posterior sample paths (abo_paths_*; include/abo_hip.h).

The reference is a dense NumPy restatement of the header's four formulas on the CPU oracle's fit (oracle.gp_oracle: fit /
kernel_matrix) — none of the library's tiling:
    φ_r(x) = sqrt(2σ_f²/R)·cos(ω_r·x/ℓ + phase_r),  f_s = c + Σ_r w[s,r]φ_r,  v_s = K̃⁻¹(y − f_s(X) − σ_n·ε_s),  g_s(z) = f_s(z) + k(z,X)·v_s
Bar of the values: measured in the test, not fixed.  The oracle takes v_s by two fp64 routes (Cholesky solve; explicit L⁻¹, then
L⁻ᵀ(L⁻¹·)); their disagreement is δ_case, and the library must be within max(100·δ_case, 1e-12) of the Cholesky route (100 × is
parity_record.MARGIN) and under the project's hard limit 1e-6, in units of sqrt(σ_f²).  Every comparison goes through
tests.parity_record.check, so the achieved error is recorded."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import thompson
from oracle import gp_oracle as O

from tests.parity_record import MARGIN, check
from tests.test_gpu_parity import FAMS, make_model

HARD = 1e-6


def data(rng, N, d):
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(axis=1) / math.sqrt(d)) + 0.3 * np.cos(5.0 * X[:, 0]) + 0.05 * rng.standard_normal(N)
    return X, y


def oracle_paths(st, y, base, Z):
    """(g by the Cholesky route (S, M), δ = max disagreement of the two routes / sqrt(σ_f²))"""
    omega, phase, w, eps = base
    sc = math.sqrt(2.0 * st.sigma_f2 / omega.shape[0])
    fX = st.mean_c + w @ (sc * np.cos(st.X @ omega.T / st.ell + phase)).T
    fZ = st.mean_c + w @ (sc * np.cos(Z @ omega.T / st.ell + phase)).T
    r = (y[None, :] - fX - math.sqrt(st.noise_var) * eps).T
    Kzx = O.kernel_matrix(st.family, st.ell, st.sigma_f2, Z, st.X)
    g1 = fZ + (Kzx @ sla.cho_solve((st.L, True), r)).T
    Linv = sla.solve_triangular(st.L, np.eye(st.L.shape[0]), lower=True, check_finite=False)
    g2 = fZ + (Kzx @ (Linv.T @ (Linv @ r))).T
    return g1, float(np.max(np.abs(g1 - g2))) / math.sqrt(st.sigma_f2)


def setup(case, family, d, N, S, R, mean_c, noise, ell, sf2=1.4, seed=0, **kw):
    rng = np.random.default_rng(1000 + seed)
    X, y = data(rng, N, d)
    model = abo.update(make_model(family, ell, sf2, noise, mean_c, **kw), X, y)
    st = O.fit(family, ell, sf2, noise, mean_c, X, y)
    base = thompson.draw_base(FAMS[family](), S, R, N, d, rng)
    return rng, X, y, model, st, base


#        name                  family d   N     M     S   R     mean  noise ell   device inputs
CASES = [("se_d2_n512",        0,     2,  512,  2051, 16, 512,  0.0,  1e-6, 0.15, False),
         ("m52_d4_n1024",      1,     4,  1024, 2048, 16, 2048, 0.7,  1e-6, 0.5,  True),
         ("m52_d8_n2048_c3",   1,     8,  2048, 2049, 64, 2048, 0.0,  1e-4, 0.9,  False),
         ("m32_d1_n5",         3,     1,  5,    333,  1,  1,    -1.5, 1e-2, 0.3,  False),
         ("m72_d16_n200",      2,     16, 200,  1000, 17, 512,  0.25, 1e-3, 1.5,  True),
         ("m32_d8_n130",       3,     8,  130,  777,  64, 2048, 0.0,  1e-5, 0.8,  False),
         ("se_d16_n300",       0,     16, 300,  515,  17, 1,    2.0,  1e-2, 1.2,  False),
         ("m72_d1_n77",        2,     1,  77,   2048, 16, 512,  0.0,  1e-4, 0.2,  True),
         ("m52_d2_n1000_c2",   1,     2,  1000, 4099, 64, 512,  0.0,  1e-6, 0.25, False),
         ("m52_d3_n61",        1,     3,  61,   1001, 16, 512,  0.5,  1e-4, 0.4,  False),     # d below its padded dimension
         ("se_d24_n150",       0,     24, 150,  700,  17, 512,  0.0,  1e-3, 1.6,  True),      # the 32-coordinate generator
         ("m32_d5_n99",        3,     5,  99,   515,  33, 64,   0.0,  1e-3, 0.7,  True)]


@pytest.mark.parametrize("name,family,d,N,M,S,R,mean_c,noise,ell,dev", CASES, ids=[c[0] for c in CASES])
def test_values_and_picks_against_the_dense_oracle(name, family, d, N, M, S, R, mean_c, noise, ell, dev):
    import torch
    rng, X, y, model, st, base = setup(name, family, d, N, S, R, mean_c, noise, ell, seed=len(name) + N)
    Z = rng.random((M, d))
    g, delta = oracle_paths(st, y, base, Z)
    bar = min(HARD, max(MARGIN * delta, 1e-12))
    paths = abo.SamplePaths(model, *base)
    Zin = torch.from_numpy(Z).cuda() if dev else Z
    vals = paths(Zin)
    k = 8
    tv, ti = paths.argmin(Zin, k=k)
    if dev:
        assert vals.is_cuda and tv.is_cuda and ti.is_cuda
        vals, tv, ti = vals.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()
    assert vals.shape == (S, M) and tv.shape == (S, k) and ti.shape == (S, k)
    err = float(np.max(np.abs(vals - g))) / math.sqrt(st.sigma_f2)
    print(f"{name}: delta_case {delta:.3e}  bar {bar:.3e}  achieved {err:.3e}")
    check("thompson_" + name, "values_over_sqrt_sf2", err, bar)
    # picks: top_val is the value at top_idx bit for bit; the ordering is abo_acq's rule on −g of the library's own values …
    assert np.array_equal(tv.view(np.int64), np.take_along_axis(vals, ti, axis=1).view(np.int64))
    skipped = 0
    for s in range(S):
        assert np.array_equal(ti[s], O.top_k(-vals[s], k)[1])
        # … and the oracle's wherever its neighbours in the order are further away than the value bar
        gs, order = O.top_k(-g[s], k + 1)
        gap = np.abs(np.diff(gs))
        for i in range(k):
            clear = gap[i] > 2.0 * bar * math.sqrt(st.sigma_f2) and (i == 0 or gap[i - 1] > 2.0 * bar * math.sqrt(st.sigma_f2))
            if clear:
                assert ti[s, i] == order[i], (s, i)
            else:
                skipped += 1
    check("thompson_" + name, "pick_comparisons_skipped_fraction", skipped / (S * k), 0.05, tighten=False)


def test_ties_nan_and_short_sets_follow_the_acquisition_rule():
    rng, X, y, model, st, base = setup("ties", 1, 4, 100, 16, 512, 0.0, 1e-3, 0.5, seed=3)
    Z0 = rng.random((300, 4))
    Z0[7, 2] = np.nan                                       # NaN first
    Z = np.concatenate([Z0, Z0[:150], Z0[100:140]])         # exact duplicates: exact ties, in other tiles and lanes
    paths = abo.SamplePaths(model, *base)
    vals = paths(Z)
    assert np.array_equal(vals[:, :150].view(np.int64), vals[:, 300:450].view(np.int64))
    assert np.all(np.isnan(vals[:, 7])) and np.all(np.isnan(vals[:, 307]))
    tv, ti = paths.argmin(Z, k=12, idx_base=1000)
    for s in range(16):
        want = O.top_k(-vals[s], 12)[1]
        assert want[0] == 7 and want[1] == 307
        assert np.array_equal(ti[s] - 1000, want)
        assert np.array_equal(tv[s, 2:].view(np.int64), vals[s, want[2:]].view(np.int64)) and np.all(np.isnan(tv[s, :2]))
    tv, ti = paths.argmin(Z0[10:15], k=8)                    # M < k: tail (NaN, −1)
    assert np.all(ti[:, 5:] == -1) and np.all(np.isnan(tv[:, 5:])) and np.all(ti[:, :5] >= 0)
    for s in range(16):
        assert sorted(ti[s, :5]) == [0, 1, 2, 3, 4]


def test_determinism_and_resident_sets():
    rng, X, y, model, st, base = setup("det", 0, 4, 333, 17, 512, 0.3, 1e-3, 0.6, seed=4)
    Z = rng.random((3001, 4))
    p1, p2 = abo.SamplePaths(model, *base), abo.SamplePaths(model, *base)
    a, b, c = p1(Z), p1(Z), p2(Z)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(a.view(np.int64), c.view(np.int64))
    sub = np.arange(5, 3001, 7)                             # a candidate's value does not depend on where it stands in the batch
    assert np.array_equal(p1(Z[sub]).view(np.int64), a[:, sub].view(np.int64))
    cands = abo.ResidentCandidates(model, Z)
    assert np.array_equal(p1(cands).view(np.int64), a.view(np.int64))
    tv0, ti0 = p1.argmin(Z, k=3)
    tv1, ti1 = p1.argmin(cands, k=3)
    assert np.array_equal(ti0, ti1) and np.array_equal(tv0.view(np.int64), tv1.view(np.int64))
    gone = sorted(set(int(j) for j in ti0[:, 0]))
    for j in gone:
        cands.exclude(j)
    v = p1(cands)
    assert np.all(np.isposinf(v[:, gone]))
    keep = np.setdiff1d(np.arange(3001), gone)
    assert np.array_equal(v[:, keep].view(np.int64), a[:, keep].view(np.int64))
    _, ti2 = p1.argmin(cands, k=3)
    assert not np.isin(ti2, gone).any()
    picks = abo.thompson_batch(model, cands, 6, R=256, rng=11)
    assert len(set(picks.tolist())) == 6 and not np.isin(picks, gone).any()
    assert np.array_equal(picks, abo.thompson_batch(model, cands, 6, R=256, rng=11))
    st_ = p1.stats()
    assert st_["S"] == 17 and st_["R"] == 512 and st_["N"] == 333 and st_["eval_ms"] > 0.0 and st_["create_ms"] > 0.0
    assert st_["eval_flop"] == 2.0 * (333 + 512) * 3001 * 17


def test_many_paths_and_chunks_agree_with_a_stable_sort_on_the_device():
    """S = 130 paths (three groups of 64 columns) over M = 300 000 candidates (two chunks), duplicates across the chunk boundary:
    per path the selection is the stable ascending order of the library's own values, and a subsample evaluated alone has the same bits"""
    import torch
    rng, X, y, model, st, base = setup("chunks", 3, 2, 64, 130, 64, 0.0, 1e-2, 0.3, seed=5)
    M = 300000
    Z = rng.random((M, 2))
    Z[200000:200500] = Z[1000:1500]
    paths = abo.SamplePaths(model, *base)
    Zd = torch.from_numpy(Z).cuda()
    vals = paths(Zd)
    tv, ti = paths.argmin(Zd, k=5)
    order = torch.sort(vals, dim=1, stable=True).indices[:, :5]
    assert torch.equal(order, ti)
    assert torch.equal(torch.gather(vals, 1, ti).view(torch.int64), tv.view(torch.int64))
    sub = np.concatenate([np.arange(0, 4096), np.arange(128890, 128900), np.arange(M - 100, M)])
    g, delta = oracle_paths(st, y, base, Z[sub])
    lib = paths(Z[sub])
    assert np.array_equal(lib.view(np.int64), vals[:, torch.from_numpy(sub).cuda()].cpu().numpy().view(np.int64))
    check("thompson_chunks", "values_over_sqrt_sf2", float(np.max(np.abs(lib - g))) / math.sqrt(st.sigma_f2),
          min(HARD, max(MARGIN * delta, 1e-12)))


def test_lifetime_append_and_refusals():
    rng, X, y, model, st, base = setup("life", 1, 2, 61, 16, 512, 0.0, 1e-3, 0.4, seed=6, n_max=128)
    Z = rng.random((500, 2))
    g, delta = oracle_paths(st, y, base, Z)
    bar = min(HARD, max(MARGIN * delta, 1e-12))
    paths = abo.SamplePaths(model, *base)
    before = paths(Z)
    model2 = abo.append(model, rng.random(2), 0.3)          # the old paths still describe the OLD model
    paths.model = None
    del model                                               # … and outlive the caller's reference to it
    import gc
    gc.collect()
    after = paths(Z)
    assert np.array_equal(before.view(np.int64), after.view(np.int64))
    check("thompson_life", "values_over_sqrt_sf2", float(np.max(np.abs(after - g))) / math.sqrt(st.sigma_f2), bar)
    assert abo.posterior_mean(model2, Z[:3]).shape == (3,)
    with pytest.raises(abo.DimensionMismatch):
        paths(rng.random((10, 3)))
    gm = abo.HipGradientGP(abo.SqExponentialKernel(), 3, 1e-3)
    Xg = rng.random((6, 2))
    gm = abo.update(gm, Xg, [[math.sin(x[0]), math.cos(x[0]), 0.0] for x in Xg])
    with pytest.raises(ValueError, match="gradient-enhanced"):
        abo.SamplePaths(gm, *thompson.draw_base(abo.SqExponentialKernel(), 16, 512, *thompson._model_shape(gm), rng))
    fresh = abo.HipStandardGP(abo.SqExponentialKernel(), 0.1)
    with pytest.raises(ValueError):
        abo.sample_paths(fresh, 4)


def test_refit_of_the_retained_handle_is_refused_not_misread():
    """abo_fit on the very handle the paths retained replaces that handle's model: a later evaluation returns ABO_EINVAL"""
    rng, X, y, model, st, base = setup("refit", 1, 2, 40, 16, 64, 0.0, 1e-3, 0.4, seed=8)
    paths = abo.SamplePaths(model, *base)
    Z = rng.random((50, 2))
    paths(Z)
    X2, y2 = data(rng, 40, 2)
    info = C.c_int64(0)
    abo._lib.check(abo._lib.lib().abo_fit(model._require(), X2.ctypes.data, 40, 2, y2.ctypes.data, abo._lib.HOST, C.byref(info)))
    with pytest.raises(ValueError, match="abo_paths_create"):
        paths(Z)
    with pytest.raises(ValueError, match="abo_paths_create"):
        paths.argmin(abo.ResidentCandidates(model, Z), k=1)


def test_device_base_arrays_and_device_outputs_of_a_resident_set():
    """abo_paths_create from base arrays in device memory, abo_paths_eval_cand into device memory: the bits of the host route"""
    import torch
    L, DEV = abo._lib.lib(), abo._lib.DEVICE
    rng, X, y, model, st, base = setup("devbase", 2, 3, 50, 16, 64, 0.2, 1e-3, 0.5, seed=9)
    Z = rng.random((777, 3))
    ref = abo.SamplePaths(model, *base)
    want, (wv, wi) = ref(Z), ref.argmin(Z, k=2)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in base]
    torch.cuda.synchronize()
    hp = C.c_void_p()
    abo._lib.check(L.abo_paths_create(model._require(), 16, 64, *[t.data_ptr() for t in dev], DEV, C.byref(hp)))
    try:
        cands = abo.ResidentCandidates(model, Z)
        vals = torch.empty((16, 777), dtype=torch.float64, device="cuda")
        tv = torch.empty((16, 2), dtype=torch.float64, device="cuda")
        ti = torch.empty((16, 2), dtype=torch.int64, device="cuda")
        abo._lib.check(L.abo_paths_eval_cand(hp, cands._h.ptr, 0, vals.data_ptr(), 2, tv.data_ptr(), ti.data_ptr(), DEV))
        assert np.array_equal(vals.cpu().numpy().view(np.int64), want.view(np.int64))
        assert np.array_equal(ti.cpu().numpy(), wi) and np.array_equal(tv.cpu().numpy().view(np.int64), wv.view(np.int64))
    finally:
        L.abo_paths_destroy(hp)


def test_c3_shape_top1_against_the_oracle_on_a_subsample():
    """C3's own shape: N = 8192, d = 8, M = 2²⁰, S = 64, R = 2048, top-1 only (no S × M array anywhere); the oracle on a 4 096-candidate
    subsample, and the arg-min over those"""
    import torch
    N, d, M, S, R = 8192, 8, 1 << 20, 64, 2048
    rng, X, y, model, st, base = setup("c3", 1, d, N, S, R, 0.0, 1e-4, 0.9, seed=7)
    Zd = torch.rand((M, d), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    paths = abo.SamplePaths(model, *base)
    tv, ti = paths.argmin(Zd, k=1)
    print("C3 shape:", paths.stats())
    sub = torch.arange(0, M, M // 4096, device="cuda")[:4096]
    Zs = Zd[sub].cpu().numpy()
    g, delta = oracle_paths(st, y, base, Zs)
    bar = min(HARD, max(MARGIN * delta, 1e-12))
    lib = paths(Zs)
    err = float(np.max(np.abs(lib - g))) / math.sqrt(st.sigma_f2)
    print(f"c3: delta_case {delta:.3e}  bar {bar:.3e}  achieved {err:.3e}")
    check("thompson_c3_shape", "values_over_sqrt_sf2", err, bar)
    tvs, tis = paths.argmin(Zs, k=1)
    skipped = 0
    for s in range(S):
        gs, order = O.top_k(-g[s], 2)
        if abs(gs[0] - gs[1]) > 2.0 * bar * math.sqrt(st.sigma_f2):
            assert tis[s, 0] == order[0]
        else:
            skipped += 1
    check("thompson_c3_shape", "pick_comparisons_skipped_fraction", skipped / S, 0.05, tighten=False)
    # the arg-min over all 2²⁰: the value of that very candidate, and no larger than the best of the subsample (a subset)
    tv, ti = tv.cpu().numpy(), ti.cpu().numpy()
    one = paths(Zd[torch.from_numpy(ti[:, 0]).cuda()].cpu().numpy())
    assert np.array_equal(np.diag(one).view(np.int64), tv[:, 0].view(np.int64))
    assert np.all(tv[:, 0] <= tvs[:, 0])
