"""The route launch_topk gives a selection of k out of M (csrc/misc.hip: topk_plan, the one function the launcher switches on), no GPU
needed: through the host-only hook abo_test_topk_plan of the test build.  What the routes compute is tests/test_gpu_select_family.py,
which asks this very hook which route a shape takes."""
import ctypes as C

import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd._lib import (TOPK_PATH_ARGMAX as ARGMAX, TOPK_PATH_BLOCKSORT as BLOCKSORT, TOPK_PATH_NONE as NONE,
                                          TOPK_PATH_SLICES as SLICES, TOPK_PATH_SMALL as SMALL)

SMALL_MAXM = 16384          # one workgroup's LDS holds that many keys
MERGE_MAX = 16384           # … and so the merge of the slices' picks
ROUND = 1024                # entries one threshold round of the block-sort chain selects
BLOCK = 2048                # scores one workgroup of that chain, and of the arg-max, takes


def plan(M, k):
    out = (C.c_int64 * 6)(*([-99] * 6))
    abo._lib.check(abo._lib.lib().abo_test_topk_plan(M, k, out))
    return dict(zip(("path", "kreal", "slice", "pairs", "rounds", "passes"), out))


def workspace(M, k):
    """topk_workspace_entries (csrc/misc.hip), what every caller allocates per buffer"""
    kp = 1
    while kp < max(1, min(k, ROUND)):
        kp *= 2
    return max(1, -(-M // BLOCK)) * kp + 2


def documented_route(M, k):
    """the rule as csrc/misc.hip documents it"""
    if k <= 0:
        return NONE
    kreal = min(k, max(M, 1))
    if kreal > ROUND:
        return BLOCKSORT
    if M <= SMALL_MAXM:
        return SMALL
    if kreal == 1:
        return ARGMAX
    return SLICES if (-(-M // SMALL_MAXM) - 1) * kreal + min(kreal, M - (-(-M // SMALL_MAXM) - 1) * SMALL_MAXM) <= MERGE_MAX else BLOCKSORT


MS = [0, 1, 2, 63, 1024, 1025, 2047, 2048, 2049, 3000, 9000, 16383, 16384, 16385, 18433, 40000, 65536, 262143, 262144, 262145, 264193,
      278528, 278529, 2 ** 20, 2 ** 20 + 2049, 2 ** 24 + 1, 2 ** 31 + 7]
KS = [-1, 0, 1, 2, 3, 100, 129, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 3072, 5000]


@pytest.mark.parametrize("M", MS)
def test_route_and_its_invariants(M):
    for k in KS + [M - 1, M, M + 3]:
        if k >= 2 ** 31:
            continue
        p = plan(M, k)
        assert p["path"] == documented_route(M, k), (M, k, p)
        if k <= 0:
            assert list(p.values()) == [NONE, 0, 0, 0, 0, 0]
            continue
        kreal = min(k, max(M, 1))
        assert p["kreal"] == kreal
        ws = workspace(M, k)
        if p["path"] == SLICES:
            sl, G = p["slice"], -(-M // p["slice"])
            assert sl >= kreal and sl <= SMALL_MAXM and sl % 2048 == 0 and G >= 2
            assert p["pairs"] == (G - 1) * kreal + min(kreal, M - (G - 1) * sl)
            assert p["pairs"] <= MERGE_MAX
            assert G * kreal <= ws - 2, (M, k, p, ws)           # slice b writes its picks at b·k: the last one ends inside the workspace
            assert (p["rounds"], p["passes"]) == (0, 0)
        elif p["path"] == ARGMAX:
            assert kreal == 1 and -(-M // BLOCK) <= ws - 2      # one partial result per block of 2048
        elif p["path"] == BLOCKSORT:
            assert p["rounds"] == -(-kreal // ROUND)
            kp = 1
            while kp < min(kreal, ROUND):
                kp *= 2
            blocks, passes = max(1, -(-M // BLOCK)), 1
            assert blocks * kp <= ws - 2                        # what the first pass leaves
            while blocks > 1:
                blocks, passes = -(-blocks * kp // BLOCK), passes + 1
            assert p["passes"] == passes
            assert (p["slice"], p["pairs"]) == (0, 0)
        else:
            assert p["path"] == SMALL and kreal <= ROUND and M <= SMALL_MAXM
            assert (p["slice"], p["pairs"], p["rounds"], p["passes"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("M,k,want", [
    (0, 1, SMALL), (0, 5, SMALL), (1, 1, SMALL), (16384, 1, SMALL), (16384, 1024, SMALL), (63, 66, SMALL),
    (16384, 1025, BLOCKSORT), (1025, 1028, BLOCKSORT), (3000, 1500, BLOCKSORT), (9000, 1025, BLOCKSORT), (9000, 3072, BLOCKSORT),
    (16385, 1, ARGMAX), (2048 * 9 + 1, 1, ARGMAX), (2 ** 20, 1, ARGMAX),
    (16385, 2, SLICES), (16385, 1024, SLICES), (40000, 100, SLICES), (65536, 100, SLICES), (262144, 1024, SLICES), (2 ** 20, 16, SLICES),
    (262145, 1024, BLOCKSORT), (262145 + 2048, 1024, BLOCKSORT), (2 ** 20 + 2049, 1024, BLOCKSORT), (2 ** 20, 100, SLICES),
])
def test_route_of_the_shapes_the_gpu_file_runs(M, k, want):
    assert plan(M, k)["path"] == want


def test_plan_details_of_the_named_shapes():
    assert plan(65536, 100) == dict(path=SLICES, kreal=100, slice=2048, pairs=3200, rounds=0, passes=0)          # the launcher's own example
    assert plan(16385, 2) == dict(path=SLICES, kreal=2, slice=2048, pairs=17, rounds=0, passes=0)                # a last slice of one entry
    assert plan(262144, 1024) == dict(path=SLICES, kreal=1024, slice=16384, pairs=16384, rounds=0, passes=0)
    assert plan(3000, 1500) == dict(path=BLOCKSORT, kreal=1500, slice=0, pairs=0, rounds=2, passes=2)
    assert plan(9000, 1025) == dict(path=BLOCKSORT, kreal=1025, slice=0, pairs=0, rounds=2, passes=4)            # 5 → 3 → 2 → 1 blocks
    assert plan(9000, 3072) == dict(path=BLOCKSORT, kreal=3072, slice=0, pairs=0, rounds=3, passes=4)
    assert plan(5, 9) == dict(path=SMALL, kreal=5, slice=0, pairs=0, rounds=0, passes=0)
    assert plan(0, 9) == dict(path=SMALL, kreal=1, slice=0, pairs=0, rounds=0, passes=0)


def test_plan_hook_refuses_a_null_output():
    assert abo._lib.lib().abo_test_topk_plan(100, 1, None) == abo._lib.ABO_EINVAL
