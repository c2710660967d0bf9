// Device arithmetic of the acquisition epilogues, shared by the posterior epilogue (misc.hip) and the refinement stage (refine.hip).
//   EI   src/acquisition_functions/ExpectedImprovement.jl:40-66   (Normal cdf = erfc(−z/√2)/2)
//   UCB  src/acquisition_functions/UpperConfidenceBound.jl:38-45
//   PI   src/acquisition_functions/ProbabilityImprovement.jl:38-63 (incl. the σ² ≤ 1e-12 → max(Δ,0) quirk)
//   GradientNormUCB  src/acquisition_functions/gradNormUCB.jl:43-51
//   EnsembleAcquisition  src/acquisition_functions/EnsembleAcq.jl:53-55  (Σ wᵢ·acqᵢ on one posterior)
//   LogEI  no reference counterpart: log EI, finite for every finite z (Ament et al. 2023)
//   MES    no reference counterpart: max-value entropy search (Wang & Jegelka 2017)
#pragma once
#include "abo_kernels.h"
#include "../../include/abo_hip.h"

namespace abo {

// Total order of Julia's stable `sortperm(scores; rev=true)` (acq_utils.jl:51): isless-descending (NaN first, then +Inf … −Inf, with
// 0.0 before −0.0), equal scores by ascending index.  Scores map to order-preserving u64 keys.
__device__ __forceinline__ uint64_t score_key(double s) {
    if (s != s) return 0xffffffffffffffffull;
    const uint64_t b = (uint64_t)__double_as_longlong(s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// the score a key came from (a NaN comes back as the canonical quiet NaN)
__device__ __forceinline__ double score_of_key(uint64_t k) {
    if (k == 0xffffffffffffffffull) return __longlong_as_double(0x7ff8000000000000ll);
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}
// true if entry (ka, ia) must come before (kb, ib)
__device__ __forceinline__ bool before(uint64_t ka, int64_t ia, uint64_t kb, int64_t ib) {
    return (ka > kb) || (ka == kb && ia < ib);
}

__device__ __forceinline__ double norm_cdf(double z) { return 0.5 * erfc(-z * 0.70710678118654752440084436210485); }
__device__ __forceinline__ double norm_pdf(double z) { return exp(-0.5 * z * z) * 0.39894228040143267793994605993438; }

// log h(z), h(z) = φ(z) + z·Φ(z) (EI = σ·h(z)), in three ranges of z; with q = Φ(z)/φ(z) the two ratios the partial derivatives
// of LogEI need come out of the same quantities, never as a quotient of two underflowed ones:
//   z > −1        h from norm_pdf / norm_cdf (φ and zΦ cancel by at most a factor 3 here; φ → 0 for large z leaves h = z)
//   −64 < z ≤ −1  q = √(π/2)·erfcx(|z|/√2), h = φ·(1 + z·q): log h = −z²/2 − ½log 2π + log1p(z·q).  1 + z·q ≈ 1/z² cancels up to
//                 12 bits at the far end, where −z²/2 ≈ −2048 carries the value: the error stays below an ulp of the sum
//   z ≤ −64       h = φ·u·S(u), q = T(u)/|z|, u = 1/z²: S = 1 − 3u + 15u² − 105u³ + 945u⁴, T = 1 − u + 3u² − 15u³ + 105u⁴ (the
//                 asymptotic series of the Mills ratio; first dropped terms 10395u⁵ < 10⁻¹⁴ and 945u⁵ < 10⁻¹⁵)
// cdf_h = Φ/h, pdf_h = φ/h.  A NaN z fails every comparison and comes out of the last range as NaN; z² overflows beyond
// |z| ≈ 1.3·10¹⁵⁴, where log h itself is below −DBL_MAX: −Inf.
constexpr double LOGEI_HALF_LOG_2PI = 0.91893853320467274178032973640562;
constexpr double LOGEI_SQRT_HALF_PI = 1.2533141373155002512078826424055;
__device__ __forceinline__ double log_h(double z, double& cdf_h, double& pdf_h) {
    if (z > -1.0) {
        const double cdf = norm_cdf(z), pdf = norm_pdf(z), h = pdf + z * cdf;
        cdf_h = cdf / h; pdf_h = pdf / h;
        return log(h);
    }
    if (z > -64.0) {
        const double q = LOGEI_SQRT_HALF_PI * erfcx(-z * 0.70710678118654752440084436210485), zq = z * q;
        pdf_h = 1.0 / (1.0 + zq); cdf_h = q * pdf_h;
        return -0.5 * z * z - LOGEI_HALF_LOG_2PI + log1p(zq);
    }
    const double z2 = z * z, u = 1.0 / z2;
    const double S = u * (-3.0 + u * (15.0 + u * (-105.0 + u * 945.0)));                  // S − 1
    const double T = 1.0 + u * (-1.0 + u * (3.0 + u * (-15.0 + u * 105.0)));
    pdf_h = z2 / (1.0 + S); cdf_h = -z * T / (1.0 + S);
    return -0.5 * z2 - LOGEI_HALF_LOG_2PI - 2.0 * log(-z) + log1p(S);
}

// ---- max-value entropy search -------------------------------------------------------------------------------------------------------
// One sample's term a(γ) = γ·φ(γ)/(2Φ(γ)) − log Φ(γ), γ = (μ − y*)/σ, and da/dγ = −(r/2)·(1 + γ² + γ·r), r = φ/Φ, in three ranges of γ.
// a ≥ 0, non-increasing, → 0 for γ → +∞ and ≈ log|γ| + ½log 2π − ½ for γ → −∞; the bracket 1 + γ² + γ·r ≈ 2/γ² there.
//   γ > −1        r = norm_pdf/norm_cdf; log Φ = log1p(−Φ(−γ)) for γ > 0 (log Φ itself would round to 0 from γ ≈ 8.3 on), log(Φ) up to
//                 0.  The bracket is taken as r + γr·(γ + r) (= r·bracket): it cancels by at most a factor 4 (at −1), and for γ beyond
//                 38.6, where φ and with it r are exactly 0, it is 0·(γ + 0) — γ² is never formed, so no 0·Inf for any finite γ.
//   −32 < γ ≤ −1  q = Φ/φ = √(π/2)·erfcx(−γ/√2), w = 1 + γq (≈ 1/γ²; log_h's quantity), r = 1/q:
//                 log Φ = −γ²/2 − ½log 2π + log q, γr/2 + γ²/2 = (γ/2q)·w, so a = (γ/2q)·w + ½log 2π − log q; bracket = 1 + (γ/q)·w.
//                 w cancels up to 10 bits at the far end and the bracket as many again (≈ 2/γ² from two terms near ∓1): relative error
//                 of a ≈ 10⁻¹³ there, of the bracket ≈ 10⁻¹⁰ — the reason the series takes over at −32 and not at log_h's −64
//   γ ≤ −32       u = 1/γ², the asymptotic series of the Mills ratio q = T(u)/|γ|, T = Σ c_k u^k, c_k = (−1)^k (2k−1)!!, to u⁸, and of the
//                 two combinations that cancel, written out so that nothing is subtracted:
//                 T = 1 + u·T₁,  T₁ = −1 + 3u − 15u² + 105u³ − 945u⁴ + 10395u⁵ − 135135u⁶ + 2027025u⁷
//                 a = T₁/(2T) + ½log 2π + log|γ| − log1p(u·T₁)
//                 bracket = u·B₁/T,  B₁ = Σ (c_{j+1} + c_{j+2}) u^j = 2 − 12u + 90u² − 840u³ + 9450u⁴ − 124740u⁵ + 1891890u⁶ − 32432400u⁷
//                 da/dγ = B₁/(2γT²)
//                 (first dropped terms at u = 2⁻¹⁰: 3.4·10⁷u⁹ < 10⁻¹⁹ in T, 6.2·10⁸u⁸ < 10⁻¹⁵ in B₁).  u is (1/γ)², which underflows to 0
//                 where γ² would overflow: a = log|γ| + ½log 2π − ½ and da/dγ = 1/γ there, finite for every finite γ.
// A NaN γ fails both comparisons and leaves the last range as NaN.
__device__ __forceinline__ double mes_a(double g, double& da) {
    if (g > -1.0) {
        const double cdf = norm_cdf(g), r = norm_pdf(g) / cdf, t = g * r;
        da = -0.5 * (r + t * (g + r));
        return 0.5 * t - (g > 0.0 ? log1p(-norm_cdf(-g)) : log(cdf));
    }
    if (g > -32.0) {
        const double q = LOGEI_SQRT_HALF_PI * erfcx(-g * 0.70710678118654752440084436210485), w = 1.0 + g * q, gr = g / q;
        da = -0.5 * (1.0 + gr * w) / q;
        return 0.5 * gr * w + LOGEI_HALF_LOG_2PI - log(q);
    }
    const double inv = 1.0 / g, u = inv * inv;
    const double T1 = -1.0 + u * (3.0 + u * (-15.0 + u * (105.0 + u * (-945.0 + u * (10395.0 + u * (-135135.0 + u * 2027025.0))))));
    const double B1 = 2.0 + u * (-12.0 + u * (90.0 + u * (-840.0 + u * (9450.0 + u * (-124740.0 + u * (1891890.0 + u * -32432400.0))))));
    const double T = 1.0 + u * T1;
    da = 0.5 * inv * B1 / (T * T);
    return 0.5 * T1 / T + LOGEI_HALF_LOG_2PI + log(-g) - log1p(u * T1);
}

// MES(μ, σ²) = (1/S)·Σ_s a(γ_s), γ_s = (μ − y*_s)/σ, summed in the order s = 0 … S − 1 by ONE lane (the scoring kernel; the refinement
// spreads the samples over a workgroup, refine.hip).  σ² ≤ 1e-12 — the library's degenerate-variance threshold, and what an excluded
// candidate (μ = +Inf, σ² = 0) carries — gives 0 with zero partials; a NaN μ or σ² gives NaN.
// PARTIALS: ∂/∂μ = (1/S)·Σ a'(γ_s)/σ, ∂/∂σ² = −(1/S)·Σ a'(γ_s)·γ_s/(2σ²)  (∂γ/∂μ = 1/σ, ∂γ/∂σ² = −γ/(2σ²))
template <bool PARTIALS>
__device__ __forceinline__ double mes_value(double mu, double var, const double* ys, int S, double& dmu, double& dvar) {
    if (var <= 1e-12) { dmu = dvar = mu != mu ? mu : 0.0; return dmu; }
    const double sg = sqrt(var);
    double f = 0.0, sa = 0.0, sb = 0.0;
    for (int s = 0; s < S; ++s) {
        const double g = (mu - ys[s]) / sg;
        double da;
        f += mes_a(g, da);
        if (PARTIALS) { sa += da; sb += da * g; }
    }
    if (PARTIALS) { dmu = sa / (sg * S); dvar = -sb / (2.0 * var * S); }
    return f / S;
}

__device__ __forceinline__ double acq_score(int kind, double mu, double var, double p0, double best_y) {
    if (kind == ABO_ACQ_UCB) return -mu + p0 * sqrt(fmax(var, 0.0));
    if (kind == ABO_ACQ_MEAN) return -mu;
    const double delta = (best_y - p0) - mu;
    if (kind == ABO_ACQ_LOGEI) {                                    // log EI: log σ + log h(z); exp of it is EI on both branches
        if (var <= 1e-12) return log(fmax(delta, 0.0));
        double a, b;
        return 0.5 * log(var) + log_h(delta / sqrt(var), a, b);
    }
    if (var <= 1e-12) return fmax(delta, 0.0);
    const double sg = sqrt(var);
    const double z = delta / sg;
    if (kind == ABO_ACQ_EI) return delta * norm_cdf(z) + sg * norm_pdf(z);
    return norm_cdf(z);
}

// acquisition value (the arithmetic of acq_score) and its partial derivatives with respect to μ and σ²
__device__ __forceinline__ double acq_value_and_partials(int kind, double mu, double var, double p0, double best_y, double& dmu,
                                                         double& dvar) {
    if (kind == ABO_ACQ_UCB) {
        const double sg = sqrt(fmax(var, 0.0));
        dmu = -1.0; dvar = var > 0.0 ? 0.5 * p0 / sg : 0.0;
        return -mu + p0 * sg;
    }
    if (kind == ABO_ACQ_MEAN) { dmu = -1.0; dvar = 0.0; return -mu; }
    const double delta = (best_y - p0) - mu;
    if (kind == ABO_ACQ_LOGEI) {                                    // ∂/∂μ = −Φ/(σ·h), ∂/∂σ² = φ/(2σ²·h)
        if (var <= 1e-12) { dmu = delta > 0.0 ? -1.0 / delta : 0.0; dvar = 0.0; return log(fmax(delta, 0.0)); }
        const double sg = sqrt(var);
        double cdf_h, pdf_h;
        const double lh = log_h(delta / sg, cdf_h, pdf_h);
        dmu = -cdf_h / sg; dvar = 0.5 * pdf_h / var;
        return 0.5 * log(var) + lh;
    }
    if (var <= 1e-12) { dmu = delta > 0.0 ? -1.0 : 0.0; dvar = 0.0; return fmax(delta, 0.0); }
    const double sg = sqrt(var), z = delta / sg, cdf = norm_cdf(z), pdf = norm_pdf(z);
    if (kind == ABO_ACQ_EI) { dmu = -cdf; dvar = 0.5 * pdf / sg; return delta * cdf + sg * pdf; }
    dmu = -pdf / sg; dvar = -0.5 * pdf * z / var;                 // PI = Φ(z)
    return cdf;
}

// Σ_t w_t·acq_t(μ, σ²) over the function-value terms (a GRADNORM_UCB term contributes nothing here).  One term of weight 1 is
// returned as is — the same bits as acq_score.
__device__ __forceinline__ double terms_score(const AcqTerms& t, double mu, double var) {
    if (t.n == 1 && t.w[0] == 1.0) return t.kind[0] == ACQ_GRADNORM_UCB ? 0.0 : acq_score(t.kind[0], mu, var, t.p0[0], t.best_y[0]);
    double f = 0.0;
    for (int i = 0; i < t.n; ++i)
        if (t.kind[i] != ACQ_GRADNORM_UCB) f = fma(t.w[i], acq_score(t.kind[i], mu, var, t.p0[i], t.best_y[i]), f);
    return f;
}

__device__ __forceinline__ double terms_value_and_partials(const AcqTerms& t, double mu, double var, double& dmu, double& dvar) {
    if (t.n == 1 && t.w[0] == 1.0) {
        if (t.kind[0] == ACQ_GRADNORM_UCB) { dmu = 0.0; dvar = 0.0; return 0.0; }
        return acq_value_and_partials(t.kind[0], mu, var, t.p0[0], t.best_y[0], dmu, dvar);
    }
    double f = 0.0;
    dmu = 0.0; dvar = 0.0;
    for (int i = 0; i < t.n; ++i) {
        if (t.kind[i] == ACQ_GRADNORM_UCB) continue;
        double a, b;
        const double v = acq_value_and_partials(t.kind[i], mu, var, t.p0[i], t.best_y[i], a, b);
        f = fma(t.w[i], v, f); dmu = fma(t.w[i], a, dmu); dvar = fma(t.w[i], b, dvar);
    }
    return f;
}

// −(mᵀm + trΣ) + β·sqrt(max(4mᵀΣm + 2‖Σ‖_F², 1e-12)) on the gradient block (outputs 1..p−1) of one point's mean m[p] and
// covariance C[p][p] (gradNormUCB.jl:43-51); the two moments are returned so that several β share them
__device__ __forceinline__ void gradnorm_moments(const double* m, const double* C, int p, double& mean_sq, double& var_sq) {
    double mm = 0.0, tr = 0.0, msm = 0.0, fro = 0.0;
    for (int q = 1; q < p; ++q) {
        mm = fma(m[q], m[q], mm);
        tr += C[q * p + q];
        double row = 0.0;
        for (int q2 = 1; q2 < p; ++q2) {
            row = fma(C[q * p + q2], m[q2], row);
            fro = fma(C[q * p + q2], C[q * p + q2], fro);
        }
        msm = fma(m[q], row, msm);
    }
    mean_sq = mm + tr;
    var_sq = 4.0 * msm + 2.0 * fro;
}
__device__ __forceinline__ double gradnorm_ucb(double mean_sq, double var_sq, double beta) {
    return -mean_sq + beta * sqrt(fmax(var_sq, 1e-12));
}

// Σ over the GRADNORM_UCB terms of w_t·gradNormUCB_{β_t}
__device__ __forceinline__ double terms_gradnorm(const AcqTerms& t, const double* m, const double* C, int p) {
    double ms, vs;
    gradnorm_moments(m, C, p, ms, vs);
    if (t.n == 1 && t.w[0] == 1.0) return t.kind[0] == ACQ_GRADNORM_UCB ? gradnorm_ucb(ms, vs, t.p0[0]) : 0.0;
    double f = 0.0;
    for (int i = 0; i < t.n; ++i)
        if (t.kind[i] == ACQ_GRADNORM_UCB) f = fma(t.w[i], gradnorm_ucb(ms, vs, t.p0[i]), f);
    return f;
}

}  // namespace abo
