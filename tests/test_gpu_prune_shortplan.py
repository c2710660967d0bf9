"""The bound pass of the pruned top-k selection on a short residue plan (csrc/ozaki.hip: "the guarded bound").

By default the bound pass contracts the first rows of L⁻¹ on 8 moduli instead of the handle's 14 and takes a proven distance δ_i off
every |V_ij| before squaring.  Every case asks for what the code claims exactly: the bounds dominate the full pass's scores (no
tolerance), and the selection is byte-identical to the path switched off and to the bound pass on the handle's own 14 moduli.  The row
scales and guards the library used are read back and compared with the Python restatement of tests/test_prune_shortplan_cpu.py.

A fitted model cannot hold a non-finite row of W (a non-finite pivot raises PosDefException), so that branch (delta = +Inf, bad_row →
a NaN sum, kept) is driven through abo_test_oz_contract_bound: the bound pass's own row-scale, quantiser, GEMM and guarded
reconstruction on a caller-made W."""
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from abstractbayesopt.jl_amd.surrogate import get_factor
from oracle import gp_oracle as O

from tests.test_gpu_parity import make_model
from tests.test_prune_shortplan_cpu import guard_delta, pow2

XI, BETA = 0.01, 2.0
N, M, K = 1536, 20000, 100


def _force(rblocks, mode):
    abo._lib.check(abo._lib.lib().abo_test_prune_force(rblocks, mode))


def _moduli(n):
    abo._lib.check(abo._lib.lib().abo_test_prune_bound_moduli(n))


@pytest.fixture(autouse=True)
def _defaults():
    _force(0, 0)
    _moduli(0)
    yield
    _force(0, 0)
    _moduli(0)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _acq(name, y):
    best = float(np.min(y))
    return {"ei": abo.ExpectedImprovement(XI, best), "logei": abo.LogExpectedImprovement(XI, best),
            "ucb": abo.UpperConfidenceBound(BETA)}[name]


def _bounds(model, m):
    ub = np.empty(m)
    abo._lib.check(abo._lib.lib().abo_test_prune_bounds(model._require(), ub.ctypes.data, m))
    return ub


def _plan(model, rows):
    sexp, delta = np.empty(rows, dtype=np.int32), np.empty(rows)
    abo._lib.check(abo._lib.lib().abo_test_prune_bound_plan(model._require(), sexp.ctypes.data, delta.ctypes.data, rows))
    return sexp, delta


def _dominates_and_selects_the_same(acq, model, Z, k, rblocks, n_b=0):
    """the short-plan bound pass (n_b = 0: the default, 8 moduli): bounds ≥ full scores without any margin, selection = path off =
    bound pass on 14 moduli; returns its statistics"""
    m = Z.shape[0]
    _force(rblocks, 0)
    _moduli(n_b)
    _, tv, ti = abo.evaluate(acq, model, Z, k=k, return_scores=False)
    st = model.prune_stats()
    assert st["bound_rows"] == 256 * max(rblocks, 1)
    ub = _bounds(model, m)
    _plan(model, st["bound_rows"])                                    # a short plan was in use
    _moduli(14)
    _, tv14, ti14 = abo.evaluate(acq, model, Z, k=k, return_scores=False)
    st14 = model.prune_stats()
    ub14 = _bounds(model, m)
    with pytest.raises(ValueError):
        _plan(model, st["bound_rows"])                                # the handle's own plan: no short plan to read back
    _moduli(0)
    _force(0, 2)
    _, tv0, ti0 = abo.evaluate(acq, model, Z, k=k, return_scores=False)
    assert model.prune_stats()["bound_rows"] == 0
    _force(0, 0)
    s, _, _ = abo.evaluate(acq, model, Z, k=0)                        # the full pass's scores
    fin = ~np.isnan(ub)
    print(f"rblocks {rblocks}: survivors {st['survivors']} (14 moduli: {st14['survivors']}), fallback {st['fallback']}, "
          f"min(bound - score) = {np.min(ub[fin] - s[fin]):.3e}, min(bound8 - bound14) = {np.min(ub[fin] - ub14[fin]):.3e}")
    assert np.array_equal(np.isnan(ub), np.isnan(ub14))
    # what prune_keep claims and the survivor list is built on (Margins)
    assert np.all(ub[fin] * (1.0 + 2.0 ** -30) + 2.0 ** -1022 - s[fin] >= 0.0)
    # and without any margin: the bound pass stores the guarded bound (misc.hip: finalize_kernel), so the inequality holds on the stored
    # numbers themselves — also where EI is subnormal and its epilogue is not monotone to the last bit
    assert np.all(ub[fin] >= s[fin])
    for tvx, tix in ((tv14, ti14), (tv0, ti0)):
        np.testing.assert_array_equal(ti, tix)
        np.testing.assert_array_equal(_bits(tv), _bits(tvx))
    return st


@pytest.fixture(scope="module")
def matern8():
    X, y = synth.standardized_problem(N, 8, 0.03)
    return y, synth.points(2, M, 8), abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8"), X, y)


@pytest.fixture(scope="module")
def se3():
    X, y = synth.standardized_problem(N, 3, 0.03)                      # d = 3: coordinates padded to dp = 4
    return y, synth.points(2, M, 3), abo.update(make_model(O.SE, 0.5, 1.5, 1e-3, contraction="int8"), X, y)


@pytest.mark.parametrize("rblocks", [0, 2])                           # the rule's R = 256, and 512: δ's row index crosses 128 and 256
@pytest.mark.parametrize("name", ["ei", "logei", "ucb"])
@pytest.mark.parametrize("which", ["matern8", "se3"])
def test_bounds_dominate_and_selection_is_unchanged(request, which, name, rblocks):
    y, Z, model = request.getfixturevalue(which)
    st = _dominates_and_selects_the_same(_acq(name, y), model, Z, K, rblocks)
    assert st["pruned"] == 1 and st["fallback"] == 0 and K <= st["survivors"] < M // 2
    assert model.timings()["oz_nmod"] == 14                           # the handle's plan, whatever the bound pass ran on


@pytest.mark.parametrize("n_b", [9, 10])                              # the other short plans the switch accepts: run-time-n reconstruction
def test_nine_and_ten_moduli(matern8, n_b):
    y, Z, model = matern8
    st = _dominates_and_selects_the_same(_acq("ei", y), model, Z, K, 2, n_b=n_b)
    assert st["pruned"] == 1 and st["fallback"] == 0 and K <= st["survivors"] < M // 2


@pytest.fixture(scope="module")
def near_duplicates():
    d = 8
    X = synth.points(1, N, d).copy()
    rng = np.random.default_rng(7)
    X[1:256:2] = X[0:255:2] + 1e-7 * rng.standard_normal((128, d))    # pairs inside the first R = 256 rows
    y = np.sin(X.sum(axis=1)) + 0.1 * np.cos(3.0 * X[:, 0])
    y = (y - y.mean()) / y.std()
    return y, synth.points(2, M, d), abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-8, contraction="int8"), X, y)


@pytest.mark.parametrize("name", ["ei", "ucb"])
def test_large_row_norms(near_duplicates, name):
    y, Z, model = near_duplicates
    Linv = get_factor(model)[2]
    l1 = np.abs(Linv[:256]).sum(axis=1)
    print(f"max ‖W_i‖₁ over the bound rows: {l1.max():.3e}")
    assert l1.max() > 1e3
    st = _dominates_and_selects_the_same(_acq(name, y), model, Z, K, 0)
    assert st["survivors"] >= K                                       # reported; it may grow with δ here
    assert st["fallback"] == (1 if st["survivors"] > M - M // 8 else 0) and st["pruned"] == 1 - st["fallback"]
    # more than 7M/8 survivors (here: all of them, a threshold of −Inf): the fallback to the full pass, same result
    acq = _acq(name, y)
    _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    _force(0, 1)
    _, tv1, ti1 = abo.evaluate(acq, model, Z, k=K, return_scores=False)
    st1 = model.prune_stats()
    _force(0, 0)
    assert st1["survivors"] == M > M - M // 8 and st1["fallback"] == 1 and st1["pruned"] == 0 and st1["bound_rows"] == 256
    np.testing.assert_array_equal(ti, ti1)
    np.testing.assert_array_equal(_bits(tv), _bits(tv1))


def test_row_scales_and_guards_match_the_restatement(matern8):
    y, Z, model = matern8
    _force(2, 0)
    abo.evaluate(_acq("ei", y), model, Z, k=K, return_scores=False)
    rows = model.prune_stats()["bound_rows"]
    assert rows == 512
    sexp, delta = _plan(model, rows)
    Linv = get_factor(model)[2]
    for i in range(rows):
        w = np.abs(Linv[i, :i + 1])
        l1 = math.fsum(w)
        s, d = guard_delta(l1, float(w.max()), i, 1.0, 8, rows)
        assert sexp[i] == s, i
        # the kernel evaluates the same expression on L1·(1 + (i+1)·2^-52) of its own fp64 row sum and closes with 1 + 2^-40
        assert d <= Fraction(float(delta[i])) <= d * (1 + (i + 1) * pow2(-50)) * (1 + pow2(-39)), (i, float(d), delta[i])
    print(f"delta: min {delta.min():.3e}, max {delta.max():.3e}; max ‖W_i‖₁ {np.abs(Linv[:rows]).sum(axis=1).max():.3e}")


@pytest.mark.parametrize("n_b", [8, 10])
def test_non_finite_row_of_w(n_b):
    """rows holding Inf / NaN: delta = +Inf, their 128-row blocks sum to NaN (as the full pass's do); the other blocks stay finite and
    are dominated by the 14-modulus contraction of the same operands"""
    import torch
    Np, Mc, rblocks, kmax = 640, 256, 2, 1.3                          # pad256(Np) = 768: the bound planes' row stride exceeds their rows
    rng = np.random.default_rng(99)
    W = np.tril(rng.standard_normal((Np, Np)) * 10.0 ** rng.uniform(-3, 3, (Np, 1)))
    W[300, 5] = np.inf                                                # block 2
    W[450, 449] = np.nan                                              # block 3
    Kz = rng.uniform(0.0, kmax, (Mc, Np))
    Wd, Kd = torch.from_numpy(W).cuda(), torch.from_numpy(Kz).cuda()
    full = torch.full((Np // 128, Mc), -1.0, dtype=torch.float64).cuda()
    got = torch.full((Np // 128, Mc), -1.0, dtype=torch.float64).cuda()
    delta = torch.full((256 * rblocks,), -1.0, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    L = abo._lib.lib()
    abo._lib.check(L.abo_test_oz_contract(0, Wd.data_ptr(), Np, Np, Np, Kd.data_ptr(), Np, Mc, kmax, 14, full.data_ptr(), Mc))
    abo._lib.check(L.abo_test_oz_contract_bound(0, Wd.data_ptr(), Np, Np, Np, Kd.data_ptr(), Np, Mc, kmax, n_b, rblocks, got.data_ptr(), Mc,
                                                delta.data_ptr()))
    full, got, delta = full.cpu().numpy(), got.cpu().numpy(), delta.cpu().numpy()
    assert np.isposinf(delta[300]) and np.isposinf(delta[450]) and np.sum(~np.isfinite(delta)) == 2 and np.all(delta >= 0.0)
    assert np.isnan(got[2:4]).all() and np.isnan(full[2:4]).all()
    assert np.isfinite(got[:2]).all() and np.all(got[:2] >= 0.0) and np.all(got[:2] <= full[:2])
    assert np.all(got[4] == -1.0)                                     # past the bound rows: not written
    print(f"n_b {n_b}: max relative shortfall of the guarded sums {np.max(1.0 - got[:2] / full[:2]):.3e}")


def test_nan_candidate_is_ranked_as_the_full_path_ranks_it():
    n, d, m = 1300, 8, 5000
    X, y = synth.standardized_problem(n, d, 0.03)
    model = abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8"), X, y)
    Z = synth.points(2, m, d).copy()
    Z[1234, 3] = np.nan
    Z[4999, 0] = np.nan
    for name in ("ei", "logei", "ucb"):
        acq = _acq(name, y)
        _, tv, ti = abo.evaluate(acq, model, Z, k=K, return_scores=False)
        assert model.prune_stats()["bound_rows"] == 256
        ub = _bounds(model, m)
        assert np.isnan(ub[1234]) and np.isnan(ub[4999]) and np.sum(np.isnan(ub)) == 2
        _force(0, 2)
        _, tv0, ti0 = abo.evaluate(acq, model, Z, k=K, return_scores=False)
        _force(0, 0)
        np.testing.assert_array_equal(ti, ti0)
        np.testing.assert_array_equal(_bits(tv), _bits(tv0))
        assert list(ti[:2]) == [1234, 4999] and np.isnan(tv[:2]).all() and not np.isnan(tv[2:]).any()


CHILD = """
import sys
import numpy as np
import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import synth
from oracle import gp_oracle as O
from tests.test_gpu_parity import make_model
X, y = synth.standardized_problem(1300, 8, 0.03)
Z = synth.points(2, 5000, 8)
model = abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8"), X, y)
abo.evaluate(abo.ExpectedImprovement(0.01, float(np.min(y))), model, Z, k=100, return_scores=False)
ub = np.empty(5000)
abo._lib.check(abo._lib.lib().abo_test_prune_bounds(model._require(), ub.ctypes.data, 5000))
sys.stdout.write(ub.tobytes().hex())
"""


def test_environment_switch_selects_the_exact_bound_pass():
    X, y = synth.standardized_problem(1300, 8, 0.03)
    Z = synth.points(2, 5000, 8)
    model = abo.update(make_model(O.MATERN52, 1.0, 1.0, 1e-3, contraction="int8"), X, y)
    acq = _acq("ei", y)
    _moduli(14)
    abo.evaluate(acq, model, Z, k=K, return_scores=False)
    ub14 = _bounds(model, 5000)
    _moduli(0)
    abo.evaluate(acq, model, Z, k=K, return_scores=False)
    ub8 = _bounds(model, 5000)
    assert not np.array_equal(_bits(ub8), _bits(ub14))                # the default is the short plan
    env = dict(os.environ, ABO_PRUNE_BOUND_MODULI="14", ABO_LIB_TEST_HOOKS="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=root, capture_output=True, text=True, check=True).stdout
    child = np.frombuffer(bytes.fromhex(out.strip().splitlines()[-1]), dtype=np.float64)
    np.testing.assert_array_equal(_bits(child), _bits(ub14))
