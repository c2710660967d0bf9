"""The guard of the fused first-level head (csrc/kgen_head32.hip), restated in NumPy float32 — no GPU.

δ_i of the file's header is evaluated here from ‖W_i‖₁, σ_f², R, dp and the full plan's constants; the fp32 dot products Ṽ = Ŵ·K̂ are formed
in forward, reverse, pairwise and blocks-of-4 order, with and without an emulated fma, on random and adversarial lower-triangular heads of W
(row L1 norms from 1 to 10⁴) and kernel columns in [0, σ_f²]:
  * |Ṽ_ij − V_ij| ≤ δ_i against the long-double product of the fp64 operands, every order;
  * S̃ = (1 − c)·Σ max(|Ṽ| − δ, 0)² ≤ the fp64 sum of squares of the fp64 products, rows in order (the full pass's form);
  * a row that leaves the fp32 range is flagged: δ = +Inf, contribution 0."""
import numpy as np
import pytest

V, U, TAU = 2.0 ** -24, 2.0 ** -53, 2.0 ** -126
R, NP, DP = 256, 8192, 8
EP_FULL, SK_FULL, N_FULL = 108, 51, 14          # the 14-modulus plan at σ_f² = 1: 2^eP ≤ P/4, rint(K·2^sK) ≤ 2⁵²


def delta_rows(W, sf2, R=R, dp=DP, eP=EP_FULL, sK=SK_FULL, nmod=N_FULL):
    """head32_prep_kernel, operation by operation"""
    kmax = sf2 * (1.0 + 2.0 ** -40)
    rec = (128.0 * nmod * nmod + 256.0 * nmod) * 2.0 ** (eP - 91)
    out = np.empty(W.shape[0])
    for i in range(W.shape[0]):
        with np.errstate(over="ignore", invalid="ignore"):
            l1 = float(np.sum(np.abs(W[i, :i + 1])))
            ok = l1 < 2.0 ** 100 and kmax < 2.0 ** 100 and l1 * kmax < 2.0 ** 100
        if not ok:
            out[i] = np.inf
            continue
        n = i + 1.0
        L = l1 * (1.0 + n * 2.0 ** -52)
        g = (R + 1.0) * V / (1.0 - (R + 1.0) * V)
        T = L * (2.0 ** -51 + 2.0 ** (54 - eP))
        sk = 2.0 ** -sK
        full = 0.5 * sk * L + 0.5 * T * n * kmax + 0.25 * n * T * sk + rec * T * sk + 2.0 * n * U * L * kmax + 2.0 ** -50 * L * kmax
        dl = L * kmax * (2.0 * V + V * V + 2.0 * (dp + 14) * U + g * (1.0 + V) * (1.0 + V)) + TAU * (2.0 * n * kmax + 2.0 * L + 3.0 * n) + full
        out[i] = dl * (1.0 + 2.0 ** -30)
    return out


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)       # one rounding (the product is exact in fp64)


def dot32(Wf, Kf, order, fma):
    """Ṽ [R][M] in float32, the products and sums in the given order"""
    Rn, M = Wf.shape[0], Kf.shape[1]

    def chain(ks):
        acc = np.zeros((Rn, M), np.float32)
        for k in ks:
            a, b = Wf[:, k:k + 1], Kf[k:k + 1, :]
            acc = _fma32(np.broadcast_to(a, (Rn, M)), np.broadcast_to(b, (Rn, M)), acc) if fma else (acc + a * b).astype(np.float32)
        return acc
    if order == "forward":
        return chain(range(Rn))
    if order == "reverse":
        return chain(range(Rn - 1, -1, -1))
    if order == "blocks4":
        acc = np.zeros((Rn, M), np.float32)
        for k0 in range(0, Rn, 4):
            acc = (acc + chain(range(k0, k0 + 4))).astype(np.float32)
        return acc
    terms = [(Wf[:, k:k + 1] * Kf[k:k + 1, :]).astype(np.float32) for k in range(Rn)]                      # pairwise
    while len(terms) > 1:
        terms = [(terms[i] + terms[i + 1]).astype(np.float32) for i in range(0, len(terms), 2)]
    return terms[0]


def _heads(rng):
    out = {}
    for target in (1.0, 30.0, 1.0e4):
        W = np.tril(rng.standard_normal((R, R)))
        W *= target / np.abs(W).sum(axis=1, keepdims=True)
        out[f"random_l1_{target:g}"] = W
    W = np.tril(rng.standard_normal((R, R)))                          # near-duplicate training points: ±large neighbours that cancel
    for i in range(1, R, 2):
        W[i, i - 1], W[i, i] = -5.0e3 * (1.0 + 1e-9 * i), 5.0e3
    out["cancelling_pairs"] = W
    W = np.tril(np.ones((R, R))) * (2.0 ** -24 + 2.0 ** -48)          # every entry rounds the same way, every product too
    out["one_sided_rounding"] = W
    W = np.tril(rng.standard_normal((R, R))) * 1e-42                  # fp32 denormals throughout
    out["denormal"] = W
    return out


@pytest.mark.parametrize("sf2", [1.0, 3.7])
def test_guard_covers_every_order(sf2):
    rng = np.random.default_rng(32)
    M = 24
    for name, W in _heads(rng).items():
        Kc = sf2 * rng.uniform(0.0, 1.0, (R, M))
        Kc[:, 0], Kc[:, 1], Kc[:, 2] = sf2, 0.0, sf2 * (1.0 - 2.0 ** -25)                                  # all ones (largest V), zeros, one-sided rounding
        Kc[:, 3] = sf2 * np.exp(-np.arange(R) * 0.4)                                                        # down into the denormals
        delta = delta_rows(W, sf2)
        Vx = W.astype(np.longdouble) @ Kc.astype(np.longdouble)
        V64 = np.zeros((R, M))
        for k in range(R):                                                                                  # an fp64 product in the generator's order
            V64 += W[:, k:k + 1] * Kc[k:k + 1, :]
        full = np.zeros(M)
        for i in range(R):                                                                                  # the full pass: rows in order, fp64
            full += V64[i] * V64[i]
        Wf, Kf = W.astype(np.float32), Kc.astype(np.float32)
        c = (NP + R + 64) * 2.0 ** -52
        worst = 0.0
        for order in ("forward", "reverse", "pairwise", "blocks4"):
            for fma in (False, True):
                if order == "pairwise" and fma:
                    continue
                Vt = dot32(Wf, Kf, order, fma)
                err = np.abs(Vt.astype(np.longdouble) - Vx).astype(np.float64)
                worst = max(worst, float(np.max(err / delta[:, None])))
                assert np.all(err <= delta[:, None]), (name, order, fma)
                t = np.maximum(np.abs(Vt.astype(np.float64)) - delta[:, None], 0.0)
                S = np.zeros(M)
                for i in range(R):
                    S += t[i] * t[i]
                S *= 1.0 - c
                assert np.all(S >= 0.0) and np.all(S <= full), (name, order, fma)
        print(f"sf2 = {sf2} {name}: max |V~ - V| / delta = {worst:.3e}")
        assert worst > 0.0 or name == "denormal"


def test_flushed_denormals_stay_inside_the_guard():
    """every denormal input, product and partial sum flushed to zero: the absolute term τ·(…) covers it"""
    rng = np.random.default_rng(5)
    W = np.tril(rng.standard_normal((R, R))) * 1e-38
    Kc = rng.uniform(0.0, 1.0, (R, 8))
    delta = delta_rows(W, 1.0)
    Vx = W.astype(np.longdouble) @ Kc.astype(np.longdouble)
    tiny = np.float32(2.0 ** -126)

    def ftz(a):
        return np.where(np.abs(a) < tiny, np.float32(0.0), a).astype(np.float32)
    Wf, Kf = ftz(W.astype(np.float32)), ftz(Kc.astype(np.float32))
    acc = np.zeros((R, 8), np.float32)
    for k in range(R):
        acc = ftz((acc + ftz(Wf[:, k:k + 1] * Kf[k:k + 1, :])).astype(np.float32))
    err = np.abs(acc.astype(np.longdouble) - Vx).astype(np.float64)
    assert np.all(err <= delta[:, None])


def test_row_out_of_range_contributes_nothing():
    rng = np.random.default_rng(6)
    W = np.tril(rng.standard_normal((R, R)))
    W[7, 3] = 1.0e200
    W[9, 0] = np.nan
    delta = delta_rows(W, 1.0)
    assert np.isinf(delta[7]) and np.isinf(delta[9]) and np.all(np.isfinite(np.delete(delta, [7, 9])))
    with np.errstate(over="ignore"):
        Wf = W.astype(np.float32)
    Wf[[7, 9]] = 0.0                                               # the preparation writes a flagged row as zeros
    Kf = rng.uniform(0.0, 1.0, (R, 4)).astype(np.float32)
    Vt = dot32(Wf, Kf, "forward", True)
    t = np.abs(Vt.astype(np.float64)) - delta[:, None]
    t = np.where(t > 0.0, t, 0.0)
    assert np.all(t[7] == 0.0) and np.all(t[9] == 0.0) and np.all(np.isfinite(t))
