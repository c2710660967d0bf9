// The μ-only tail of the FIRST bound level of the pruned top-k selection in fp32 (acq.hip: prune_select).
//
// kgen_tail.hip's job — μ̃_tail = σ_f²·Σ_{k ≥ R} α_k·κ̃(r̃²_jk) for every candidate, with a PROVEN ε_j ≥ |μ̃_j − μ_j| — and its mapping
// (16 candidates per workgroup in LDS, two training points per lane in registers, sweep over k from k0, fixed-order reduction, a lane
// past the last training point sits the step out), with the pair arithmetic in packed fp32.  The first level runs over all M
// candidates and its mean has one consumer, an upper bound of the score whose survivors are all evaluated again by the full
// pipeline: a looser mean costs survivors and nothing else, and the second level is there if they become many.
//   * operands: the same scaled fp64 inputs x = Xs_k, z = Z_j·s, each rounded once to fp32.  z: once per workgroup, into LDS.  x: once
//     per bound pass, by tail32_stage_kernel below, into the pair-interleaved image Xf that a lane fills its registers from with
//     16-byte loads.  (The rows of Xs are the same for every workgroup, chunk and candidate; on the benchmark's problem 65 536
//     workgroups a pass each read them as fp64 and rounded them again.  ABO_TAIL32_STAGE=0, STAGED = false, keeps that: the same
//     values either way, so μ̃_tail and ε are bit-identical.)  The lane's two training points are the halves of a packed register
//     pair, the candidate's coordinate is broadcast to both halves;
//   * distance in the DIFFERENCE form, one v_pk_add_f32 and one v_pk_fma_f32 per coordinate and two pairs (the expanded form's
//     cancellation would cost 4(dp + 2)·2⁻²⁴·w ≈ 6·10⁻⁵ per pair at w = 16);
//   * kappa_tail32 (abo_kappa.h): v_sqrt_f32, v_exp_f32, the polynomial in packed fp32;
//   * the product with σ_f²·α_k and the running sum in fp64: v_cvt_f64_f32 (exact) and one v_fma_f64 per pair — an fp32 running sum
//     over terms of L1 norm 10⁵ would alone put more than 0.1 into ε.
//
// The guard.  v = 2⁻²⁴, u = 2⁻⁵³, w_j = max_{k ≥ R}|x_k|² + |z_j|² (fp64, as in kgen_tail.hip), r = |x − z| the exact distance of the fp64
// inputs, κ(r) the exact kernel value.  The derivation assumes the compiler's default kernel mode, fp32 denormals KEPT by the adds,
// fmas and conversions (v_sqrt_f32 and v_exp_f32 flush in any mode: abo_kappa.h); the absolute term TAIL32_R_ABS below is sized so
// that the bound also holds with every fp32 denormal flushed.
//   (a) input rounding.  x̂_c = x_c(1 + δ), ẑ_c = z_c(1 + δ'), |δ|, |δ'| ≤ v: x̂ − ẑ = (x − z) + Δ, |Δ| ≤ v(|x| + |z|) ≤ v·√(2w) (Euclidean norms;
//       (a + b)² ≤ 2(a² + b²)).  This term is ABSOLUTE in r — it does not shrink when x and z are close.
//   (b) difference and fma chain.  ê_c = (x̂_c − ẑ_c)(1 + δ''), |δ''| ≤ v; the chain adds dp non-negative terms ê_c², each passing at most dp
//       roundings: r̃² = Σ ê_c²(1 + θ_c), |θ_c| ≤ dp·v(1 + dp·v).  Hence √r̃² = |ê|(1 + θ'), |θ'| ≤ dp·v/2·(1 + dp·v), and |ê| within a factor
//       1 ± v of |x̂ − ẑ|:   |√r̃² − r| ≤ (dp/2 + 1)·v₁·r + v₁·√(2w),   v₁ = v(1 + 2⁻¹⁰) (the second-order terms; dp ≤ 32).
//       Underflow: a coordinate, a difference or a square below 2⁻¹²⁶ loses at most 2⁻¹⁴⁹ when denormals are kept; flushed, the
//       squares lose at most dp·2⁻¹²⁶ of r̃² (√ of it: 2⁻⁶⁰·⁵ of r̃), coordinates and differences 2⁻¹²⁶ each: together below
//       TAIL32_R_ABS = 2⁻⁵⁹ in r̃.  Overflow: w < TAIL_W_MAX = 2⁴⁰ keeps |x̂_c|, |ẑ_c| < 2²⁰·⁵ and r̃² < 2⁴² (and q·d̃ of ν = 7/2 below 2⁶³).
//   (c) κ's sensitivity to r (abo_kappa.h): a relative change ρ of r moves κ by at most TAIL32_REL_R·|ln(1 + ρ)|, an absolute one by
//       TAIL32_LIP_R per unit.  With (b): |κ(√r̃²) − κ(r)| ≤ TAIL32_REL_R·(dp/2 + 1)·v₁ + TAIL32_LIP_R·(v₁·√(2w) + TAIL32_R_ABS).
//   (d) evaluation.  |kappa_tail32(r̃²) − κ(√r̃²)| ≤ TAIL32_ETA_EVAL (abo_kappa.h: sqrt and exp to the ISA's 1 ulp, exponent, polynomial,
//       product).  The conversion to fp64 is exact.
//       η_j = TAIL32_ETA_EVAL + TAIL32_REL_R·(dp/2 + 1)·v₁ + TAIL32_LIP_R·(v₁·√(2w_j) + TAIL32_R_ABS) bounds |κ̃ − κ| for every pair of
//       candidate j.
//   (e) unchanged from kgen_tail.hip, (c) – (e) there: the full launch's own distance to κ, η_full = (dp + 14)·u per pair; the two fp64
//       summations in different fixed orders, (2Np + 32)·u·σ_f²·‖α‖₁ (|κ̃| ≤ 1 + 2⁻²⁰ here, inside the 1.0001 below); the epilogue's rounding.
//   ε_j = 1.0001·σ_f²·[(η_j + η_full)·Σ_{k ≥ R}|α_k| + (2Np + 64)·u·‖α‖₁] + 8u·|mean_c| — the shape of kgen_tail.hip's, with another η_j.
//   On the benchmark's problem (d = 8, unit box, ℓ = 1… w ≤ 16): η = (16 + 3.7 + 3.6)·v = 1.39·10⁻⁶.
// Non-finite and out-of-range input: the rule of kgen_tail.hip, decided in fp64 — !(w < TAIL_W_MAX) (a NaN or ±Inf coordinate
// included) gives μ̃_tail = NaN, and the candidate is kept.  Whatever the fp32 pairs of such a candidate produced (Inf − Inf, 0·Inf)
// is dropped with it; within a candidate inside the range no pair can be non-finite.
#include "kgen_core.h"

namespace abo {

typedef float f4_t __attribute__((ext_vector_type(4)));

// Xf of kgen_core.h: one thread per pair of training points and coordinate
__global__ void __launch_bounds__(256) tail32_stage_kernel(const double* __restrict__ Xs, int N, int dp, int k0, float* __restrict__ Xf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int pr = i / dp, c = i - pr * dp;
    const int k = k0 + 2 * pr;
    if (k >= N) return;
    const int k1 = k + 1 < N ? k + 1 : 0;
    *reinterpret_cast<f2_t*>(Xf + ((int64_t)pr * dp + c) * 2) = f2_t{(float)Xs[(int64_t)k * dp + c], (float)Xs[(int64_t)k1 * dp + c]};
}

hipError_t launch_tail32_stage(const double* Xs, int N, int dp, int k0, float* Xf, hipStream_t s) {
    if (k0 < 0 || k0 % 128 || k0 >= N || dp <= 0) return hipErrorInvalidValue;
    const int64_t n = (int64_t)((N - k0 + 1) / 2) * dp;
    hipLaunchKernelGGL(tail32_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Xs, N, dp, k0, Xf);
    return hipGetLastError();
}

template <int FAM, int DP, bool STAGED>
__global__ void __launch_bounds__(256) kgen_tail32_kernel(KgenTailArgs p) {
    __shared__ __attribute__((aligned(16))) float zs[JT][DP];          // fl32(z)
    __shared__ double zz[JT];                                          // |z|² (fp64: the guard's w)
    __shared__ double red[4][JT];
    const int t = threadIdx.x;
    const int jb = blockIdx.x * JT;
    if (t < JT) {
        const int64_t gj = p.j0 + jb + t;
        double q = 0.0;
        for (int c = 0; c < DP; ++c) {
            const double z = (c < p.d && gj < p.M) ? p.Z[gj * p.d + c] * p.s : 0.0;
            zs[t][c] = (float)z;
            q = fma(z, z, q);
        }
        zz[t] = q;
    }
    __syncthreads();

    double mu[JT];
#pragma unroll
    for (int jj = 0; jj < JT; ++jj) mu[jj] = 0.0;

    for (int k0 = p.k0; k0 < p.Np; k0 += KSTEP) {
        const int k = k0 + 2 * t;
        if (k < p.N) {
            // a column past the last training point reads row 0 with weight 0 (kgen_tail.hip: no padding row of Xs or alpha is read)
            const bool in1 = k + 1 < p.N;
            f2_t x[DP];
            if constexpr (STAGED) {
                const float* xf = p.Xf + (int64_t)(k - p.k0) * DP;          // (k − k0 even: 2·DP floats from a multiple of 2·DP)
                if constexpr (DP >= 2) {
#pragma unroll
                    for (int c = 0; c < DP; c += 2) {
                        const f4_t v = *reinterpret_cast<const f4_t*>(xf + 2 * c);
                        x[c] = f2_t{v[0], v[1]};
                        x[c + 1] = f2_t{v[2], v[3]};
                    }
                } else {
                    x[0] = *reinterpret_cast<const f2_t*>(xf);
                }
            } else {
                const double* xp0 = p.Xs + (int64_t)k * DP;
                const double* xp1 = p.Xs + (int64_t)(in1 ? k + 1 : 0) * DP;
                if constexpr (DP >= 2) {
#pragma unroll
                    for (int c = 0; c < DP; c += 2) {
                        const d2_t v0 = *reinterpret_cast<const d2_t*>(xp0 + c);
                        const d2_t v1 = *reinterpret_cast<const d2_t*>(xp1 + c);
                        x[c] = f2_t{(float)v0[0], (float)v1[0]};
                        x[c + 1] = f2_t{(float)v0[1], (float)v1[1]};
                    }
                } else {
                    x[0] = f2_t{(float)xp0[0], (float)xp1[0]};
                }
            }
            const double a0 = p.alpha[k] * p.sigma_f2, a1 = in1 ? p.alpha[k + 1] * p.sigma_f2 : 0.0;
#pragma unroll
            for (int jj = 0; jj < JT; ++jj) {
                asm volatile("" ::: "memory");          // keep the candidates in LDS (see kgen_rows)
                f2_t r{0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < DP; ++c) {
                    const float z = zs[jj][c];
                    const f2_t e = x[c] - f2_t{z, z};
                    r = __builtin_elementwise_fma(e, e, r);
                }
                const f2_t kv = kappa_tail32<FAM>(r);
                mu[jj] = fma((double)kv[1], a1, fma((double)kv[0], a0, mu[jj]));
            }
        }
    }
    // fixed-order reduction: lanes (xor tree) → 4 waves (serial)
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int jj = 0; jj < JT; ++jj) {
        double v = mu[jj];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) red[wave][jj] = v;
    }
    __syncthreads();
    const int64_t gj = p.j0 + jb + t;
    if (t < JT && gj < p.M) {
        const double u = 0x1p-53, v1 = 0x1p-24 * (1.0 + 0x1p-10);
        const double a_tail = p.norms[0], a_all = p.norms[1];
        const double w = p.norms[2] + zz[t];
        const double eta = TAIL32_ETA_EVAL + TAIL32_REL_R * (0.5 * DP + 1.0) * v1 + TAIL32_LIP_R * (v1 * __builtin_sqrt(2.0 * w) + TAIL32_R_ABS);
        const double sum = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        p.mu_tail[gj] = w < TAIL_W_MAX ? sum : __longlong_as_double(0x7ff8000000000000ll);
        // (an out-of-range w makes ε meaningless — possibly NaN or Inf: the candidate is kept on μ̃ = NaN alone)
        p.eps[gj] = 1.0001 * p.sigma_f2 * ((eta + (DP + 14) * u) * a_tail + (2.0 * p.Np + 64.0) * u * a_all) + 8.0 * u * __builtin_fabs(p.mean_c);
    }
}

template <int FAM, bool STAGED>
static hipError_t launch_tail32_dp(const KgenTailArgs& a, hipStream_t s) {
    dim3 grid(a.Mc / JT), block(256);
    switch (a.dp) {
        case 1: hipLaunchKernelGGL((kgen_tail32_kernel<FAM, 1, STAGED>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((kgen_tail32_kernel<FAM, 2, STAGED>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((kgen_tail32_kernel<FAM, 4, STAGED>), grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL((kgen_tail32_kernel<FAM, 8, STAGED>), grid, block, 0, s, a); break;
        case 16: hipLaunchKernelGGL((kgen_tail32_kernel<FAM, 16, STAGED>), grid, block, 0, s, a); break;
        case 32: hipLaunchKernelGGL((kgen_tail32_kernel<FAM, 32, STAGED>), grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_kgen_tail32(const KgenTailArgs& a, hipStream_t s) {
    if (a.Mc <= 0) return hipSuccess;
    // the conditions of launch_kgen_tail
    if (a.Mc % JT || a.k0 < 0 || a.k0 % 128 || a.k0 >= a.N || a.N > a.Np) return hipErrorInvalidValue;
    switch (a.family) {
        case ABO_KERNEL_SE: return a.Xf ? launch_tail32_dp<ABO_KERNEL_SE, true>(a, s) : launch_tail32_dp<ABO_KERNEL_SE, false>(a, s);
        case ABO_KERNEL_MATERN52: return a.Xf ? launch_tail32_dp<ABO_KERNEL_MATERN52, true>(a, s) : launch_tail32_dp<ABO_KERNEL_MATERN52, false>(a, s);
        case ABO_KERNEL_MATERN72: return a.Xf ? launch_tail32_dp<ABO_KERNEL_MATERN72, true>(a, s) : launch_tail32_dp<ABO_KERNEL_MATERN72, false>(a, s);
        case ABO_KERNEL_MATERN32: return a.Xf ? launch_tail32_dp<ABO_KERNEL_MATERN32, true>(a, s) : launch_tail32_dp<ABO_KERNEL_MATERN32, false>(a, s);
        default: return hipErrorInvalidValue;
    }
}

// test hook: out[i] = kappa_tail32(family, fl32(d2[i])), both halves of the pair given the same argument and required to agree
__global__ void kappa_tail32_test_kernel(int family, const double* d2, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = (float)d2[i];
    const f2_t q{x, x};
    f2_t v;
    if (family == ABO_KERNEL_SE) v = kappa_tail32<ABO_KERNEL_SE>(q);
    else if (family == ABO_KERNEL_MATERN52) v = kappa_tail32<ABO_KERNEL_MATERN52>(q);
    else if (family == ABO_KERNEL_MATERN72) v = kappa_tail32<ABO_KERNEL_MATERN72>(q);
    else v = kappa_tail32<ABO_KERNEL_MATERN32>(q);
    out[i] = (v[0] == v[1] || (v[0] != v[0] && v[1] != v[1])) ? (double)v[0] : __longlong_as_double(0x7ff8000000000000ll);
}

hipError_t launch_kappa_tail32_test(int family, const double* d2, double* out, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kappa_tail32_test_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, family, d2, out, n);
    return hipGetLastError();
}

}  // namespace abo
