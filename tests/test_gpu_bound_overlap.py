"""The fp32 tail of the first bound level of the pruned top-k selection on training points staged once per pass in fp32
(ABO_TAIL32_STAGE): csrc/posterior.hip, csrc/kgen_tail32.hip; DESIGN.md §3b-1.

The switch may not change a bit of anything.  It is read once per process, so each of its two settings runs the cases of
tests/bound_overlap_child.py in a child process of its own (both at the same time, once per module), and 0 — the tail rounding its
operands itself — is the reference:
  * N = 640 (a head of 256 rows, a tail of 384), d = 8 and 3 (padding coordinates), Matérn-5/2 and SE, EI, M = 20 000 (no multiple of the
    chunk or of 64), k = 100: the selection, and μ̃, ε, head and sum of squares of every candidate, bit for bit — with the statistics
    that show the fused head and the fp32 tail ran;
  * N = 641 (the last training point has no partner) and N = 513 (a tail of one full pair row and one point);
  * a candidate with a NaN coordinate is kept under both settings;
  * in this process, with the default: a model updated between two calls — the staged image is written by every pass, never kept."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import abstractbayesopt.jl_amd as abo
from oracle import gp_oracle as O

from tests import bound_overlap_child as child
from tests.test_gpu_parity import make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [0, 1]                                                     # ABO_TAIL32_STAGE; the first is the reference
SHAPES = ["m52_d8", "se_d8", "m52_d3", "se_d3"]
ODD = ["odd_n641", "odd_n513"]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.fixture(scope="module")
def runs():
    """{stage: the child's arrays}"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for stg in SETTINGS:
            env = dict(os.environ, ABO_TAIL32_STAGE=str(stg), ABO_LIB_TEST_HOOKS="1")
            path = os.path.join(tmp, f"s{stg}.npz")
            flags = ["-s"] if sys.flags.no_user_site else []
            cmd = [sys.executable, *flags, os.path.join(ROOT, "tests", "bound_overlap_child.py"), path]
            procs.append((stg, path, subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        for key, path, p in procs:
            try:
                log, _ = p.communicate(timeout=600)
            except subprocess.TimeoutExpired:
                for _, _, q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, f"child {key}: exit {p.returncode}\n{log[-4000:]}"
            with np.load(path) as z:
                out[key] = {k: z[k] for k in z.files}
    return out


@pytest.fixture(autouse=True)
def _defaults():
    def reset():
        lib = abo._lib.lib()
        abo._lib.check(lib.abo_test_prune_force(0, 0))
        abo._lib.check(lib.abo_test_prune_levels(0, -1))
    reset()
    yield
    reset()


def _took_the_fused_first_level(r, name):
    pruned, bound_rows, level1_rows = (int(v) for v in r[f"{name}.stats"])
    assert pruned == 1 and bound_rows == 256 and level1_rows == 256          # (head and sum of squares were read back: the fused head ran)


def _same_selection(r, ref, name):
    np.testing.assert_array_equal(r[f"{name}.top_idx"], ref[f"{name}.top_idx"])
    np.testing.assert_array_equal(_bits(r[f"{name}.top_val"]), _bits(ref[f"{name}.top_val"]))


def _same_bounds(r, ref, name):
    for what in ("mu", "eps", "head", "ssq"):
        np.testing.assert_array_equal(_bits(r[f"{name}.{what}"]), _bits(ref[f"{name}.{what}"]), err_msg=f"{name}: {what}")


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("setting", SETTINGS[1:])
def test_selection_unchanged_byte_for_byte(runs, setting, name):
    for key in (setting, SETTINGS[0]):
        _took_the_fused_first_level(runs[key], name)
    _same_selection(runs[setting], runs[SETTINGS[0]], name)
    assert np.all(np.isfinite(runs[setting][f"{name}.top_val"]))


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("setting", SETTINGS[1:])
def test_bounds_unchanged(runs, setting, name):
    _same_bounds(runs[setting], runs[SETTINGS[0]], name)
    r = runs[setting]
    assert np.all(np.isfinite(r[f"{name}.mu"])) and np.all(r[f"{name}.eps"] > 0.0) and np.all(r[f"{name}.ssq"] >= 0.0)


@pytest.mark.parametrize("name", ODD)
@pytest.mark.parametrize("setting", SETTINGS[1:])
def test_odd_n_and_the_pair_partner(runs, setting, name):
    for key in (setting, SETTINGS[0]):
        _took_the_fused_first_level(runs[key], name)
    _same_selection(runs[setting], runs[SETTINGS[0]], name)
    _same_bounds(runs[setting], runs[SETTINGS[0]], name)
    assert np.all(np.isfinite(runs[setting][f"{name}.mu"]))


def test_odd_n_last_point_counts(runs):
    """the staged image of the last, partnerless point carries its weight: without it μ̃ would miss the full pass's mean by more than ε"""
    name = "odd_n641"
    X, y, Z = child.problem(name)
    model = abo.update(make_model(O.MATERN52, 1.0, child.SF2, child.NOISE, contraction="int8"), X, y)
    mu, _ = abo.mean_and_var(model, Z)
    for key in SETTINGS:
        r = runs[key]
        assert np.all(np.abs(r[f"{name}.mu"] - mu) <= r[f"{name}.eps"])


@pytest.mark.parametrize("setting", SETTINGS)
def test_nan_candidate_is_kept(runs, setting):
    r = runs[setting]
    _took_the_fused_first_level(r, "nan")
    assert int(r["nan.top_idx"][0]) == child.NAN_ROW and np.isnan(r["nan.top_val"][0]) and not np.isnan(r["nan.top_val"][1:]).any()
    assert np.isnan(r["nan.mu"][child.NAN_ROW])
    _same_selection(r, runs[SETTINGS[0]], "nan")
    _same_bounds(r, runs[SETTINGS[0]], "nan")


def _fit(name):
    N, d, fam, ell, _ = child.CASES[name]
    X, y, Z = child.problem(name)
    return abo.update(make_model(getattr(O, fam), ell, child.SF2, child.NOISE, contraction="int8"), X, y), Z, y


def _equal_to(got, r, name):
    np.testing.assert_array_equal(got["top_idx"], r[f"{name}.top_idx"])
    np.testing.assert_array_equal(_bits(got["top_val"]), _bits(r[f"{name}.top_val"]))
    for what in ("mu", "eps", "head", "ssq"):
        np.testing.assert_array_equal(_bits(got[what]), _bits(r[f"{name}.{what}"]), err_msg=what)


def test_update_between_two_calls(runs):
    """a pruned call, then at once a model that grew by one point (the staged image changes size and content, the storage may move), then a
    pruned call on it: equal to the same call with the path off; then a fresh handle on the recycled context: the child's figures"""
    X, y, Z = child.problem("odd_n641")
    acq = abo.ExpectedImprovement(child.XI, float(np.min(y)))
    m1 = abo.update(make_model(O.MATERN52, 1.0, child.SF2, child.NOISE, contraction="int8"), X[:640], y[:640])
    child.force_first_level(abo)
    first = child.pruned_call(abo, m1, Z, y[:640])
    assert list(first["stats"]) == [1, 256, 256]
    m2 = abo.update(m1, X, y)
    got = child.pruned_call(abo, m2, Z, y)
    assert list(got["stats"]) == [1, 256, 256]
    abo._lib.check(abo._lib.lib().abo_test_prune_force(0, 2))
    _, tv0, ti0 = abo.evaluate(acq, m2, Z, k=child.K, return_scores=False)
    assert m2.prune_stats()["bound_rows"] == 0
    np.testing.assert_array_equal(got["top_idx"], ti0)
    np.testing.assert_array_equal(_bits(got["top_val"]), _bits(tv0))
    del m1, m2
    m3, Z3, y3 = _fit("odd_n641")
    child.force_first_level(abo)
    _equal_to(child.pruned_call(abo, m3, Z3, y3), runs[SETTINGS[0]], "odd_n641")
