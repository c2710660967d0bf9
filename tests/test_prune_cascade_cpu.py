"""Host-side plan of the two bound levels of the pruned top-k selection (csrc/acq.hip: prune_plan): a first level of
N/32 rows over all candidates, the N/8 pass on its survivors.  No GPU needed: abo_test_prune_plan_levels of the test build is plain host
code.  The four values abo_test_prune_plan has always returned are what tests/test_acq_prune_cpu.py pins; they are compared here with
what the new call returns next to the first level's row blocks."""
import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo

EI = 0
M, K = 1 << 20, 100


def _force(rblocks, mode=0):
    abo._lib.check(abo._lib.lib().abo_test_prune_force(rblocks, mode))


def _levels(pre_rblocks, level2_min=-1):
    abo._lib.check(abo._lib.lib().abo_test_prune_levels(pre_rblocks, level2_min))


@pytest.fixture(autouse=True)
def _defaults():
    _force(0)
    _levels(0)
    yield
    _force(0)
    _levels(0)


def plan_levels(rows, m=M, k=K):
    out = np.zeros(5, dtype=np.int64)
    abo._lib.check(abo._lib.lib().abo_test_prune_plan_levels(rows, m, k, 0, EI, 0.01, 1, 1, 8, out.ctypes.data))
    return [int(v) for v in out]


def plan_old(rows, m=M, k=K):
    out = np.zeros(4, dtype=np.int64)
    abo._lib.check(abo._lib.lib().abo_test_prune_plan(rows, m, k, 0, EI, 0.01, 1, 1, 8, out.ctypes.data))
    return [int(v) for v in out]


@pytest.mark.parametrize("rows,rblocks0", [(1536, 0), (2048, 0), (3072, 1), (4096, 1), (8192, 1), (16384, 2), (65536, 8)])
def test_first_level_is_a_thirty_second_of_the_factor_rounded_to_256(rows, rblocks0):
    assert plan_levels(rows)[4] == rblocks0


@pytest.mark.parametrize("rows", [257, 512, 1300, 1536, 2048, 2303, 2304, 3071, 3072, 4096, 5000, 8192, 12288, 16384, 30000, 65536, 1 << 20])
def test_a_first_level_is_below_the_bound_pass_or_absent(rows):
    eligible, rblocks, _, _, rblocks0 = plan_levels(rows)
    assert eligible and rblocks >= 1
    assert rblocks0 == 0 or 1 <= rblocks0 < rblocks
    if rblocks == 1:
        assert rblocks0 == 0


@pytest.mark.parametrize("rows,m", [(1300, M), (1536, M), (2048, M), (3072, M), (4096, M), (8192, M), (16384, M), (65536, M),
                                    (1536, 20000), (1300, 5000), (8192, 4095), (256, M)])
def test_the_four_old_values_are_unchanged(rows, m):
    assert plan_levels(rows, m)[:4] == plan_old(rows, m)
    expect = {1300: 1, 1536: 1, 2048: 1, 3072: 2, 4096: 2, 8192: 4, 16384: 8, 65536: 32}      # tests/test_acq_prune_cpu.py
    if rows in expect:
        assert plan_old(rows, m)[1] == expect[rows]
    assert plan_old(rows, m)[2] == 1024 and plan_old(rows, m)[3] == m - m // 8
    _levels(-1)
    assert plan_levels(rows, m)[:4] == plan_old(rows, m)


def test_a_forced_bound_pass_has_no_first_level_unless_asked_for():
    assert plan_levels(8192) == [1, 4, 1024, M - M // 8, 1]
    for rb in (1, 2, 3, 4, 6, 8):
        _force(rb)
        assert plan_levels(8192) == [1, rb, 1024, M - M // 8, 0]
    _force(2)
    _levels(1)
    assert plan_levels(1536, 20000) == [1, 2, 1024, 17500, 1]
    _force(0)
    assert plan_levels(8192)[4] == 1 and plan_levels(16384)[4] == 1          # forced below the rule's 2 at N = 16384
    _levels(2)
    assert plan_levels(8192)[4] == 2                                          # N/16 at N = 8192
    _levels(-1)
    assert plan_levels(8192)[4] == 0 and plan_levels(65536)[4] == 0


def test_a_forced_first_level_must_be_below_the_bound_pass():
    lib = abo._lib.lib()
    out = np.zeros(5, dtype=np.int64)
    _levels(4)
    assert lib.abo_test_prune_plan_levels(8192, M, K, 0, EI, 0.01, 1, 1, 8, out.ctypes.data) == abo._lib.ABO_EINVAL
    assert "not below" in abo._lib.last_error()
    _levels(1)
    assert lib.abo_test_prune_plan_levels(1536, M, K, 0, EI, 0.01, 1, 1, 8, out.ctypes.data) == abo._lib.ABO_EINVAL      # rblocks = 1
    _levels(3)
    assert plan_levels(8192)[4] == 3
    assert lib.abo_test_prune_levels(-2, -1) == abo._lib.ABO_EINVAL and lib.abo_test_prune_levels(0, -2) == abo._lib.ABO_EINVAL
    assert plan_levels(8192)[4] == 3                                          # a refused call changes nothing


def test_binding_and_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "abo_hip.h")).read()
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr)                     # a new entry point only
    assert re.search(r"\bint32_t\s+abo_get_prune_levels\s*\(", hdr) and "abo_get_prune_levels" in abo._lib.EXPORTS
    for name in ("abo_test_prune_levels", "abo_test_prune_plan_levels"):
        assert name in abo._lib.TEST_EXPORTS
    import ctypes as C
    assert C.sizeof(abo._lib.AboPruneStats) == 64
    assert hasattr(abo.HipStandardGP, "prune_levels")
