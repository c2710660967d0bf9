"""Host-side decisions of the pruned top-k selection (csrc/acq.hip: prune_plan; DESIGN.md "Pruned top-k selection"): when the path is
taken, how many row blocks of L⁻¹ the bound pass contracts, how many candidates set the threshold and when the survivor pass gives
way to the ordinary full pass.  No GPU needed: abo_test_prune_plan of the test build is plain host code."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EI, UCB, PI, MEAN = 0, 1, 2, 3


def plan(rows, M, k, want_scores=0, kind=EI, p0=0.01, p_out=1, int8=1, d=8):
    out = np.zeros(4, dtype=np.int64)
    abo._lib.check(abo._lib.lib().abo_test_prune_plan(rows, M, k, want_scores, kind, p0, p_out, int8, d, out.ctypes.data))
    return {"eligible": bool(out[0]), "rblocks": int(out[1]), "k0": int(out[2]), "max_survivors": int(out[3])}


def test_kind_constants_match_the_library():
    assert (abo.ExpectedImprovement(0.0, 0.0).kind, abo.UpperConfidenceBound(1.0).kind, abo.ProbabilityImprovement(0.0, 0.0).kind) == (EI, UCB, PI)
    assert C.sizeof(abo._lib.AboPruneStats) == 5 * 8 + 3 * 8


def test_headline_shape_is_eligible():
    p = plan(8192, 1 << 20, 100)
    assert p == {"eligible": True, "rblocks": 4, "k0": 1024, "max_survivors": (1 << 20) - (1 << 17)}


@pytest.mark.parametrize("rows,rblocks", [(1300, 1), (1536, 1), (2048, 1), (3072, 2), (4096, 2), (8192, 4), (16384, 8), (65536, 32)])
def test_row_blocks_are_an_eighth_of_the_factor_rounded_to_256(rows, rblocks):
    assert plan(rows, 1 << 20, 100)["rblocks"] == rblocks


@pytest.mark.parametrize("k,k0", [(1, 1024), (100, 1024), (256, 1024), (257, 1028), (1000, 4000)])
def test_threshold_set_size(k, k0):
    assert plan(8192, 1 << 20, k)["k0"] == k0


def test_every_condition_is_needed():
    base = dict(rows=8192, M=1 << 20, k=100)
    assert plan(**base)["eligible"]
    assert plan(**base, kind=UCB, p0=2.0)["eligible"] and plan(**base, kind=UCB, p0=0.0)["eligible"]
    assert not plan(**base, kind=UCB, p0=-1.0)["eligible"]            # UCB falls with σ for β < 0
    assert not plan(**base, kind=PI)["eligible"] and not plan(**base, kind=MEAN)["eligible"]
    assert not plan(**base, want_scores=1)["eligible"]
    assert not plan(**{**base, "k": 0})["eligible"]
    assert not plan(**base, p_out=9)["eligible"]                       # gradient-enhanced model
    assert not plan(**base, int8=0)["eligible"]                        # fp64 engine (or planes the generator does not write)
    assert not plan(256, 1 << 20, 100)["eligible"]                     # one row block: nothing to leave out
    assert plan(257, 1 << 20, 100)["eligible"]


def test_floor_on_the_candidate_count():
    assert not plan(8192, 4095, 100)["eligible"] and plan(8192, 4096, 100)["eligible"]          # 4·K0, K0 = 1024
    assert not plan(8192, 15999, 1000)["eligible"] and plan(8192, 16000, 1000)["eligible"]      # K0 = 4k


def test_fallback_threshold_is_seven_eighths():
    assert plan(1536, 20000, 100)["max_survivors"] == 17500
    assert plan(1300, 5000, 100)["max_survivors"] == 4375


def test_environment_switch_turns_the_path_off():
    code = ("import numpy as np, abstractbayesopt.jl_amd as abo\n"
            "o = np.zeros(4, dtype=np.int64)\n"
            "abo._lib.check(abo._lib.lib().abo_test_prune_plan(8192, 1 << 20, 100, 0, 0, 0.01, 1, 1, 8, o.ctypes.data))\n"
            "print(int(o[0]))\n")
    for val, want in (("0", "0"), ("1", "1")):
        env = dict(os.environ, ABO_ACQ_PRUNE=val, ABO_LIB_TEST_HOOKS="1", PYTHONPATH=ROOT)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
        assert out.strip().splitlines()[-1] == want
