// Device math of the kernel families: k(x, z) = sigma_f2 · kappa(‖x − z‖² / ell²), evaluated with the library's own exp and
// sqrt sequences (no libm calls).  Shared by the kernel-matrix generator (kgen.hip) and the fused small-N fit (chol.hip) so
// that both produce the same bits for the same pair of points.
// Reference: [upstream KernelFunctions] SqExponentialKernel / Matern52Kernel / Matern32Kernel; ApproxMatern52Kernel and
// ApproxMatern72Kernel, src/surrogates/GradientGP.jl:94-101, :320-327.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/abo_hip.h"

namespace abo {

// exp(x) for x ≤ 0 (all the kernel families need): Cody–Waite reduction x = n·ln2 + r, |r| ≤ ln2/2,
// degree-12 Taylor polynomial (remainder 1.7e-16 relative), ldexp.  18 fp64 instructions with no
// compare/select chain; underflow falls out of v_ldexp_f64 (→ 0 below 2⁻¹⁰⁷⁴).  Measured against
// mpmath in tests/test_gpu_parity.py::test_kappa_device_math (≤ 2 ulp).
__device__ __forceinline__ double exp_nonpos(double x) {
    const double n = rint(x * 1.4426950408889634074);
    double r = fma(n, -6.93147180369123816490e-01, x);     // ln2 hi (32 trailing zero bits)
    r = fma(n, -1.90821492927058770002e-10, r);            // ln2 lo
    double p = 2.08767569878680989792e-09;                 // 1/12!
    p = fma(p, r, 2.50521083854417187751e-08);
    p = fma(p, r, 2.75573192239858906526e-07);
    p = fma(p, r, 2.75573192239858906526e-06);
    p = fma(p, r, 2.48015873015873015873e-05);
    p = fma(p, r, 1.98412698412698412698e-04);
    p = fma(p, r, 1.38888888888888888889e-03);
    p = fma(p, r, 8.33333333333333333333e-03);
    p = fma(p, r, 4.16666666666666666667e-02);
    p = fma(p, r, 1.66666666666666666667e-01);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// sqrt(x) for finite x ≥ 0: v_rsq_f64 seed + two coupled Newton steps (Goldschmidt form) + one residual
// correction; x below 1e-290 (kernel value indistinguishable from κ(0)) returns 0 instead of 0·inf.  NaN stays NaN (the compare is
// false for it and g is NaN already): a candidate with a non-finite coordinate must not come out with a finite kernel value.
__device__ __forceinline__ double sqrt_pos(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    const double e = fma(-g, g, x);
    g = fma(e, h, g);
    return x <= 1e-290 ? 0.0 : g;
}

// ---- the μ-only tail of the pruned selection's bound pass (kgen_tail.hip) ----------------------------------------------------------
// Shorter sequences whose result only has to stay within a PROVEN distance of kappa_eval (the bound pass subtracts that distance from
// its mean); nothing that is returned to a caller is computed with them.
//
// TAIL_ETA_EVAL bounds |kappa_tail(r²) − κ(r²)| for one finite r² ≥ TAIL_R2_MIN handed to both, in units of κ(0) = 1, u = 2⁻⁵³:
//   sqrt   g̃ = √r²·(1 + δ_s): v_rsq_f64 is specified to 2²⁹ ulp (2⁻²³ relative); a seed error e, |e| ≤ 2⁻²², leaves 1.5e² ≤ 1.5·2⁻⁴⁴
//          after the one coupled step, plus 4u of rounding.  Only the odd powers of the Matérn polynomial and the exponent are built
//          from g̃, the even powers from r² itself, so κ moves by the PARTIAL derivative at fixed r²: with a = c·√r²,
//          |a·∂κ/∂a|·δ_s = a²e⁻ᵃ ≤ 0.55 (ν = 3/2), (a² + a³/3)e⁻ᵃ ≤ 0.94 (ν = 5/2), (a³/3 + a⁴/15)e⁻ᵃ ≤ 0.74 (ν = 7/2), none for
//          SE: below 0.94·(1.5·2⁻⁴⁴ + 4u) < 1.42·2⁻⁴⁴ = 8.1·10⁻¹⁴.
//   exp    the argument t = −c·g̃ is rounded (|t|·u·eᵗ ≤ 0.37u), clamped at −800 (e⁻⁸⁰⁰ < 2⁻¹⁰⁷⁴: both sides of the clamp give 0), the
//          reduction r = t − n·ln2 is exact to 2u (|n| ≤ 1155),
//          the degree-10 Taylor polynomial on |r| ≤ ln2/2 leaves |r|¹¹/11!·e^{|r|} ≤ 2.17·10⁻¹³·1.4143 < 3.1·10⁻¹³ relative, Horner adds
//          10u: the factor eᵗ carries at most 3.2·10⁻¹³ < 2⁻⁴¹·⁵ relative, and q·eᵗ = κ ≤ 1.
//   rest   the Matérn polynomial q and the product: below 6u.
// Together below 3.2·10⁻¹³ + 8.1·10⁻¹⁴ + 6u < 4.02·10⁻¹³ < 2⁻⁴¹ = 4.55·10⁻¹³.
// TAIL_LIP: κ is Lipschitz in r² — |dκ/dr²| ≤ 1/2 (SE), 3/2 (ν = 3/2), 5/6 (ν = 5/2), 7/10 (ν = 7/2), each attained at r² = 0 — so an
// absolute error δ of the squared distance (the expansion's cancellation, the clamp at TAIL_R2_MIN) costs at most 1.5·δ.
constexpr double TAIL_ETA_EVAL = 0x1p-41;
constexpr double TAIL_LIP = 1.5;
constexpr double TAIL_R2_MIN = 0x1p-200;       // clamp of the expanded squared distance: no negative argument, no 0·∞ from the rsq seed
constexpr double TAIL_W_MAX = 0x1p40;          // |x|² + |z|² (scaled) up to which the guard is stated: r² ≤ 2·TAIL_W_MAX stays far inside the
                                               // range of the rsq seed and of the distance's error term

// exp(x) for any x ≤ 0 (NaN is taken for −800: the caller answers for non-finite input): exp_nonpos with the polynomial cut at degree
// 10 and the argument clamped where the result is 0 anyway, which keeps n inside the int range
__device__ __forceinline__ double exp_nonpos_tail(double x) {
    x = __builtin_fmax(x, -800.0);
    const double n = rint(x * 1.4426950408889634074);
    double r = fma(n, -6.93147180369123816490e-01, x);
    r = fma(n, -1.90821492927058770002e-10, r);
    double p = 2.75573192239858906526e-07;                 // 1/10!
    p = fma(p, r, 2.75573192239858906526e-06);
    p = fma(p, r, 2.48015873015873015873e-05);
    p = fma(p, r, 1.98412698412698412698e-04);
    p = fma(p, r, 1.38888888888888888889e-03);
    p = fma(p, r, 8.33333333333333333333e-03);
    p = fma(p, r, 4.16666666666666666667e-02);
    p = fma(p, r, 1.66666666666666666667e-01);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}

// sqrt(x) for TAIL_R2_MIN ≤ x < 2⁴²: the seed and ONE coupled step, no residual correction; NaN and +Inf come back as NaN
__device__ __forceinline__ double sqrt_tail(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    const double g = x * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    return fma(g, r, g);
}

// κ(r²) without σ_f², r² the expanded squared distance before the clamp
template <int FAM>
__device__ __forceinline__ double kappa_tail(double d2) {
    d2 = __builtin_fmax(d2, TAIL_R2_MIN);
    if constexpr (FAM == ABO_KERNEL_SE) {
        return exp_nonpos_tail(-0.5 * d2);
    } else if constexpr (FAM == ABO_KERNEL_MATERN52) {
        const double s5 = 2.23606797749978969640917366873128;
        const double d = sqrt_tail(d2);
        return fma(d2, 5.0 / 3.0, fma(s5, d, 1.0)) * exp_nonpos_tail(-s5 * d);
    } else if constexpr (FAM == ABO_KERNEL_MATERN72) {
        const double s7 = 2.64575131106459059050161575363926;
        const double d = sqrt_tail(d2);
        return fma(d2 * d, 7.0 * s7 / 15.0, fma(d2, 14.0 / 5.0, fma(s7, d, 1.0))) * exp_nonpos_tail(-s7 * d);
    } else {
        const double s3 = 1.73205080756887729352744634150587;
        const double d = sqrt_tail(d2);
        return fma(s3, d, 1.0) * exp_nonpos_tail(-s3 * d);
    }
}

// ---- the same tail in fp32, for the M-wide first bound level (kgen_tail32.hip) ------------------------------------------------------
// Two pairs at a time in the halves of a packed register pair: v_sqrt_f32 and v_exp_f32 per half, the Matérn polynomial and the
// products in packed fp32.  Nothing that is returned to a caller is computed with it either.
//
// TAIL32_ETA_EVAL bounds |kappa_tail32(q) − κ(√q)| for one fp32 number 0 ≤ q < 2·TAIL_W_MAX handed to both as the squared distance,
// in units of κ(0) = 1, v = 2⁻²⁴ (fp32 unit roundoff; products of two of the errors below, ≤ (16v)², are covered by the slack left):
//   d̃ = v_sqrt_f32(q) = √q·(1 + δ_s), |δ_s| ≤ 2v: the ISA documents 1 ulp, and an ulp is at most 2⁻²³ of the value.
//   p̃  the Matérn polynomial, every term positive, so its relative error is at most the worst term's: each fma and each constant
//      rounded to fp32 gives v, a factor d̃ gives 2v, the cubic term is (q·d̃)·c₃ (ONE factor d̃, one more product):
//      ν = 3/2: 1 + c·d̃: 4v;  ν = 5/2: the linear term through two fmas: 5v;  ν = 7/2: the linear term through three: 6v;  SE: no p.
//   t̃ = fl(c̃·d̃), c̃ = fl(−√(2ν)·log₂e): t̃ = t·(1 + θ), |θ| ≤ 2v + v + v = 4v (SE: t̃ = fl(c̃·q): 2v).  With a = √(2ν)·√q (SE: q/2),
//      2^t̃ = e⁻ᵃ·e^{−aθ}: the value moves by at most a·κ·|θ|, and a·κ(a) ≤ 0.84 (ν = 3/2), 1.18 (5/2), 1.45 (7/2), 0.37 (SE).
//      The clamp at TAIL32_T_MIN changes nothing: 2^t is below 2⁻¹⁴⁹ there, 0 in fp32 on either side of it.
//   Ẽ = v_exp_f32(t̃) = 2^t̃·(1 + δ_e), |δ_e| ≤ 2v (1 ulp again).  The instruction flushes a denormal result: an absolute 2⁻¹²⁶ times
//      p̃ < 2⁶² — nothing.  A denormal q is flushed by v_sqrt_f32 (d̃ = 0, κ̃ = 1, κ ≥ 1 − 2⁻⁶³): nothing either.
//   κ̃ = fl(p̃·Ẽ): one more v.
// |κ̃ − κ| ≤ κ·(θ_p + 2v + v) + a·κ·4v: 4 + 3 + 3.4 = 10.4v (ν = 3/2), 5 + 3 + 4.7 = 12.7v (5/2), 6 + 3 + 5.8 = 14.8v (7/2), 2 + 0.74 = 2.8v (SE):
// below 16v = 2⁻²⁰ for every family.
// The distance the kernel hands over is an fp32 r̃² whose root is off by a relative and an absolute amount (kgen_tail32.hip), so the
// guard needs κ's sensitivity to r, not to r²: |r·dκ/dr| ≤ 0.74 (SE 2/e; ν = 3/2: 0.55, 5/2: 0.61, 7/2: 0.64) and |dκ/dr| ≤ 0.64 (SE e^{−1/2} =
// 0.607; ν = 3/2: √3/e = 0.638, 5/2: 0.627, 7/2: 0.622).  tests/test_kgen_tail32_cpu.py checks all of these figures numerically.
constexpr double TAIL32_ETA_EVAL = 0x1p-20;
constexpr double TAIL32_REL_R = 0.74;
constexpr double TAIL32_LIP_R = 0.64;
constexpr double TAIL32_R_ABS = 0x1p-59;       // absolute slack of r̃ for fp32 underflow anywhere in the distance (kgen_tail32.hip)
constexpr float TAIL32_T_MIN = -150.0f;        // clamp of the exponent handed to v_exp_f32

typedef float f2_t __attribute__((ext_vector_type(2)));

// 2^t per half, t ≤ 0 (NaN is taken for TAIL32_T_MIN: the caller answers for non-finite input)
__device__ __forceinline__ f2_t exp2_tail32(f2_t t) {
    return f2_t{__builtin_amdgcn_exp2f(__builtin_fmaxf(t[0], TAIL32_T_MIN)), __builtin_amdgcn_exp2f(__builtin_fmaxf(t[1], TAIL32_T_MIN))};
}

// κ(√q) per half without σ_f², q the squared distance of the difference form (never negative)
template <int FAM>
__device__ __forceinline__ f2_t kappa_tail32(f2_t q) {
    constexpr double L2E = 1.44269504088896340736;          // (the constants: rounded ONCE to fp32)
    if constexpr (FAM == ABO_KERNEL_SE) {
        constexpr float c = (float)(-0.5 * L2E);
        return exp2_tail32(q * f2_t{c, c});
    } else {
        const f2_t d{__builtin_amdgcn_sqrtf(q[0]), __builtin_amdgcn_sqrtf(q[1])};
        const f2_t one{1.0f, 1.0f};
        if constexpr (FAM == ABO_KERNEL_MATERN52) {
            constexpr float s5 = 2.23606797749978969640917366873128f, c = (float)(-2.23606797749978969640917366873128 * L2E), c2 = (float)(5.0 / 3.0);
            const f2_t p = __builtin_elementwise_fma(q, f2_t{c2, c2}, __builtin_elementwise_fma(d, f2_t{s5, s5}, one));
            return p * exp2_tail32(d * f2_t{c, c});
        } else if constexpr (FAM == ABO_KERNEL_MATERN72) {
            constexpr float s7 = 2.64575131106459059050161575363926f, c = (float)(-2.64575131106459059050161575363926 * L2E), c2 = (float)(14.0 / 5.0);
            constexpr float c3 = (float)(7.0 * 2.64575131106459059050161575363926 / 15.0);
            const f2_t p = __builtin_elementwise_fma(q * d, f2_t{c3, c3},
                                                     __builtin_elementwise_fma(q, f2_t{c2, c2}, __builtin_elementwise_fma(d, f2_t{s7, s7}, one)));
            return p * exp2_tail32(d * f2_t{c, c});
        } else {
            constexpr float s3 = 1.73205080756887729352744634150587f, c = (float)(-1.73205080756887729352744634150587 * L2E);
            return __builtin_elementwise_fma(d, f2_t{s3, s3}, one) * exp2_tail32(d * f2_t{c, c});
        }
    }
}

template <int FAM>
__device__ __forceinline__ double kappa_eval(double d2) {
    if constexpr (FAM == ABO_KERNEL_SE) {
        return exp_nonpos(-0.5 * d2);
    } else if constexpr (FAM == ABO_KERNEL_MATERN52) {
        // (1 + √5 d + 5 d²/3) e^{−√5 d}; closed form also covers the reference's Taylor branch
        // (src/surrogates/GradientGP.jl:94-101) to 1e-16.  5 d²/3 is a multiplication by the rounded
        // constant 5/3: ≤1 ulp from the reference's division (a 14-instruction fp64 divide otherwise)
        const double s5 = 2.23606797749978969640917366873128;
        const double d = sqrt_pos(d2);
        return fma(d2, 5.0 / 3.0, fma(s5, d, 1.0)) * exp_nonpos(-s5 * d);
    } else if constexpr (FAM == ABO_KERNEL_MATERN72) {
        // src/surrogates/GradientGP.jl:320-327
        const double s7 = 2.64575131106459059050161575363926;
        const double d = sqrt_pos(d2);
        return fma(d2 * d, 7.0 * s7 / 15.0, fma(d2, 14.0 / 5.0, fma(s7, d, 1.0))) * exp_nonpos(-s7 * d);
    } else {
        const double s3 = 1.73205080756887729352744634150587;
        const double d = sqrt_pos(d2);
        return fma(s3, d, 1.0) * exp_nonpos(-s3 * d);
    }
}

}  // namespace abo
