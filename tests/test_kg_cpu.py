"""Knowledge gradient over a discrete decision set, host side — no device work.

The checker is tests/kg_oracle.py (Frazier, Powell and Dayanik 2009, Algorithm 1).  Here: the checker against an independent quadrature
of E[max] and against closed cases, its invariances, the places that name the new entry point (header, ctypes binding, Julia shim), the
refusal of a null handle without a device, the host's argument checks and its chunk merge with the library call stubbed, and the
input-quality condition of the GPU cases (tests/test_gpu_kg.py), computed with the checker."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import abstractbayesopt.jl_amd as abo
from abstractbayesopt.jl_amd import surrogate as S
from oracle import gp_oracle as O
from tests import kg_oracle as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "integration", "julia", "KnowledgeGradient.jl")
HEADER = os.path.join(ROOT, "include", "abo_hip.h")
QUAD_TOL = 1e-9          # the trapezoid rule's own error at the step of kg_quadrature, for |b| of order 1 (measured against the two-line closed form below)


def planted(n, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    if n >= 5:
        b[1], b[n - 1], a[2] = b[3], b[0], a[4]              # duplicate slopes, a duplicate intercept
    return a, b


@pytest.mark.parametrize("n", [1, 2, 3, 5, 130, 257])
def test_oracle_against_quadrature(n):
    for seed in range(3):
        a, b = planted(n, 10 * n + seed)
        v, q = K.kg_lines(a, b), K.kg_quadrature(a, b)
        print(n, seed, v, q, abs(v - q))
        assert v >= 0.0 and abs(v - q) <= QUAD_TOL


def test_closed_cases():
    assert K.kg_lines([0.7], [-1.3], with_count=True) == (0.0, 1, False)
    assert K.kg_lines([0.1, -2.0, 3.0], [0.5, 0.5, 0.5], with_count=True) == (0.0, 1, False)
    for (a1, b1), (a2, b2) in (((0.3, -0.4), (-0.2, 1.1)), ((1.0, 2.0), (1.0, -2.0)), ((5.0, 0.1), (-5.0, 0.3))):
        db, da = abs(b1 - b2), a1 - a2
        want = db * K.h(-abs(da / db))
        v, n, _ = K.kg_lines([a1, a2], [b1, b2], with_count=True)
        assert n == 2 and abs(v - want) <= 4e-16 * max(1.0, want)
        assert abs(K.kg_quadrature([a1, a2], [b1, b2]) - want) <= QUAD_TOL
    # the tangents of a parabola: every line is on the envelope
    b = np.linspace(-3.0, 3.0, 257)
    v, n, tie = K.kg_lines(-0.5 * b * b, b, with_count=True)
    assert n == 257 and not tie and abs(v - K.kg_quadrature(-0.5 * b * b, b)) <= QUAD_TOL
    # one dominating steep line, last in the order: it pops the stack down to the line of the lowest slope
    rng = np.random.default_rng(4)
    a2, b2 = rng.standard_normal(300), rng.uniform(-1.0, 1.0, 300)
    a2[0], b2[0] = 1e9, 2.0
    assert K.kg_lines(a2, b2, with_count=True)[1] == 2
    assert math.isnan(K.kg_lines([0.0, np.nan], [1.0, 2.0])) and math.isnan(K.kg_lines([0.0, 1.0], [np.inf, 2.0]))


@pytest.mark.parametrize("n", [3, 130])
def test_invariances(n):
    a, b = planted(n, n)
    v = K.kg_lines(a, b)
    assert v >= 0.0
    perm = np.random.default_rng(1).permutation(n)
    assert K.kg_lines(a[perm], b[perm]) == v                       # the order in memory does not matter: one sorted order
    assert abs(K.kg_lines(a, -b) - v) <= 1e-14 * max(1.0, v)       # Z is symmetric
    assert abs(K.kg_lines(a + 3.25, b) - v) <= 1e-14 * max(1.0, v)


def test_header_binding_and_shim_name_the_same_function():
    from tests import test_julia_shim_cpu as J
    protos = J.c_prototypes()
    name = "abo_acq_kg"
    assert name in protos and name in abo._lib.EXPORTS
    assert protos[name] == [("abo_gp", 1), ("double", 1), ("int64_t", 0), ("double", 1), ("int64_t", 0), ("int32_t", 0), ("int32_t", 0),
                            ("double", 0), ("int32_t", 0), ("int64_t", 0), ("double", 1), ("int32_t", 0), ("double", 1), ("int64_t", 1),
                            ("int32_t", 0)]
    want = {("abo_gp", 1): C.c_void_p, ("double", 1): C.c_void_p, ("int64_t", 1): C.c_void_p, ("int64_t", 0): C.c_int64,
            ("int32_t", 0): C.c_int32, ("double", 0): C.c_double}
    assert list(abo._lib.lib().abo_acq_kg.argtypes) == [want[p] for p in protos[name]]
    assert abo._lib.lib().abo_acq_kg.restype is C.c_int32
    calls = J.julia_calls(JL)
    assert len(calls) == 1 and calls[0][0] == name
    code = J._strip_jl_comments(open(JL).read())
    assert len(re.findall(r"LIBABO\.\w+\(", code)) == 1
    _, types, ret, line = calls[0]
    assert ret == "Int32" and len(types) == len(protos[name])
    assert all(J.jl_matches_c(t, c) for t, c in zip(types, protos[name])), line
    assert 'include("KnowledgeGradient.jl")' in open(J.SHIMS[0]).read()
    hdr = open(HEADER).read()
    assert re.search(r"#define ABO_ABI_VERSION 7\b", hdr) and re.search(r"enum \{ ABO_KG_SELF = 1 \}", hdr) and abo._lib.KG_SELF == 1
    block = hdr[hdr.index("#define ABO_ABI_VERSION"):]
    block = block[:block.index("*/")]
    assert name in block[block.index("added within ABI 7"):]
    assert "abo_test_kg_lines" in abo._lib.TEST_EXPORTS


def test_null_handle_is_refused_without_a_device():
    L = abo._lib.lib()
    assert L.abo_acq_kg(None, None, 1, None, 0, 1, 0, -1.0, 0, 0, None, 0, None, None, 0) == abo._lib.ABO_EINVAL
    msg = abo._lib.last_error()
    assert "abo_acq_kg" in msg and "null" in msg


class _Unreachable:
    def __call__(self):
        raise AssertionError("the library was touched")


def _fitted_stub(model, d):
    model._h = S._Handle(None)
    model._d = d
    return model


def test_host_checks_raise_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(abo._lib, "lib", _Unreachable())
    m = _fitted_stub(abo.HipStandardGP(1.7 * abo.with_lengthscale(abo.Matern52Kernel(), 0.3), 1e-2), 3)
    x3, x2 = np.zeros((4, 3)), np.zeros((4, 2))
    for call in (lambda: abo.knowledge_gradient(m, x2), lambda: abo.knowledge_gradient(m, x3, x2), lambda: abo.KnowledgeGradient()(m, x2)):
        with pytest.raises(abo.DimensionMismatch):
            call()
    g = _fitted_stub(abo.HipGradientGP(abo.Matern52Kernel(), 4, 0.1), 3)
    sh = abo.HipShardedGP(abo.Matern52Kernel(), 0.1, devices=(0, 0))
    for bad, word in ((g, "gradient"), (sh, "sharded")):
        for call in (lambda: abo.knowledge_gradient(bad, x3), lambda: abo.KnowledgeGradient(decision=x3)(bad, x3)):
            with pytest.raises(TypeError, match=word):
                call()
    with pytest.raises(ValueError, match="8192"):
        abo.knowledge_gradient(m, x3, np.zeros((8193, 3)))                 # more than 8192 decision points
    with pytest.raises(ValueError, match="8192"):
        abo.knowledge_gradient(m, np.zeros((8193, 3)))                     # the symmetric form is one call
    for bad_noise in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise"):
            abo.knowledge_gradient(m, x3, noise=bad_noise)
    with pytest.raises(ValueError, match="negative"):
        abo.knowledge_gradient(m, x3, k=-1)
    with pytest.raises(TypeError, match="KnowledgeGradient"):
        abo.EnsembleAcquisition([1.0], [abo.KnowledgeGradient()])
    with pytest.raises(AssertionError, match="touched"):
        abo.knowledge_gradient(m, x3)


class _StubLib:
    """abo_acq_kg answered on the host: score of candidate i = a function of its first coordinate; the selection in the library's order"""

    def __init__(self):
        self.calls = []

    def __call__(self):
        return self

    def abo_acq_kg(self, h, za, ma, zb, mb, d, zs, noise, flags, idx_base, scores, k, tv, ti, outs):
        z = np.ctypeslib.as_array(C.cast(za, C.POINTER(C.c_double)), shape=(ma, d))
        s = np.round(np.abs(np.sin(7.0 * z[:, 0])), 1)                      # many exact ties, across chunks too
        self.calls.append((ma, mb, noise, flags, idx_base, k))
        np.ctypeslib.as_array(C.cast(scores, C.POINTER(C.c_double)), shape=(ma,))[:] = s
        if k > 0:
            v, i = S._host_top_k(s, k)
            np.ctypeslib.as_array(C.cast(tv, C.POINTER(C.c_double)), shape=(k,))[:] = v
            np.ctypeslib.as_array(C.cast(ti, C.POINTER(C.c_int64)), shape=(k,))[:] = np.where(i >= 0, i + idx_base, -1)
        return 0


def test_chunks_and_their_merge_with_the_library_stubbed(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(abo._lib, "lib", stub)
    monkeypatch.setattr(S, "KG_CHUNK", 64)
    m = _fitted_stub(abo.HipStandardGP(1.7 * abo.with_lengthscale(abo.Matern52Kernel(), 0.3), 1e-2), 2)
    rng = np.random.default_rng(0)
    za, zb = rng.random((150, 2)), rng.random((9, 2))
    for k in (0, 5, 70, 150):
        stub.calls.clear()
        r = abo.knowledge_gradient(m, za, zb, noise=0.25, k=k)
        assert [(c[0], c[4]) for c in stub.calls] == [(64, 0), (64, 64), (22, 128)]
        assert all(c[1] == 9 and c[2] == 0.25 and c[3] == abo._lib.KG_SELF and c[5] == min(k, c[0]) for c in stub.calls)
        sc = r if k == 0 else r[0]
        want = np.round(np.abs(np.sin(7.0 * za[:, 0])), 1)
        assert np.array_equal(sc, want)
        if k:
            ov, oi = K.top_k(want, k)
            assert np.array_equal(r[2], oi) and np.array_equal(r[1], ov)
    stub.calls.clear()
    abo.knowledge_gradient(m, za[:10], zb, include_self=False)
    abo.knowledge_gradient(m, za[:10])
    assert stub.calls == [(10, 9, -1.0, 0, 0, 0), (10, 0, -1.0, 0, 0, 0)]
    v, i = S._host_top_k(np.array([1.0, np.nan, 3.0, 3.0]), 6)
    assert np.array_equal(i, [1, 2, 3, 0, -1, -1]) and np.isnan(v[0]) and np.all(np.isnan(v[4:]))


@pytest.mark.parametrize("form", ["rect", "self"])
@pytest.mark.parametrize("N,d,noise,ell", K.GP_CASES)
def test_gpu_cases_are_informative(N, d, noise, ell, form):
    """The inputs of tests/test_gpu_kg.py must exercise the scan: at least half of the 130 candidates with KG ≥ 1e-6·√σ_f² and a median
    envelope of ≥ 4 lines — held here for the decision set given, without and with the candidate's own line (the Python host's
    default), Matérn-5/2.  The symmetric form is printed beside them: its rows have 130 lines, not 257, and its median envelope is 3 to 4."""
    X, y = K.gp_problem(N, d)
    za, zb = K.gp_queries(d)
    v, n, _ = K.kg_model(O.MATERN52, ell, K.SF2, noise, K.MEAN_C, X, y, za, zb, include_self=form == "self")
    share, med = float(np.mean(v >= 1e-6 * math.sqrt(K.SF2))), float(np.median(n))
    vs, ns, _ = K.kg_model(O.MATERN52, ell, K.SF2, noise, K.MEAN_C, X, y, za)
    print((N, d, ell, form), {"share": share, "median_env": med, "sym_share": float(np.mean(vs >= 1e-6 * math.sqrt(K.SF2))), "sym_median_env": float(np.median(ns))})
    assert share >= 0.5 and med >= 4.0
