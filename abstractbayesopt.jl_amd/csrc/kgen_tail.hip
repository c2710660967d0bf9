// The μ-only tail of the bound pass of the pruned top-k selection (acq.hip: prune_select).
//
// The bound pass needs the residue planes of K_XZ for the first R = res_kmax training columns only, but the posterior mean needs every
// column.  For the columns k ≥ R the kernel values have one consumer: μ, which in that pass is used for one thing, an upper bound of
// the score.  So this kernel computes μ̃_tail = σ_f²·Σ_{k ≥ R} α_k·κ̃(r̃²_jk) with cheaper arithmetic (36 instead of 57 fp64 instructions
// per pair at dp = 8, Matérn-5/2) and hands the epilogue a PROVEN ε_j ≥ |μ̃_j − μ_j|, μ_j being what the full launch computes:
//   * r̃² = |x|² + |z|² − 2x·z: |x|² once per lane and sweep step, |z|² and −2z once per workgroup, dp + 1 instructions per pair
//     instead of 2·dp;
//   * kappa_tail (abo_kappa.h): one coupled step on the rsq seed, a degree-10 polynomial in the exponential;
//   * σ_f² once per lane and sweep step (folded into α), no mask multipliers (a lane past the last training point sits the step
//     out), no non-finite check per pair (see below).
// Same mapping as kgen_kernel: 16 candidates per workgroup in LDS, two training points per lane in registers, fixed-order reduction.
//
// The guard.  Both launches see the same rounded inputs x = Xs_k, z = Z_j·s; let κ_jk be the exact kernel value on them, u = 2⁻⁵³,
// w_j = max_{k ≥ R}|x_k|² + |z_j|².
//   (a) distance.  |x|², |z|² by fma chains: relative error dp·u each.  The sum chain (one addition, dp fmas) has partial sums bounded
//       by |x|² + |z|² + 2Σ|x_c z_c| ≤ 2(|x|² + |z|²), one rounding each: |r̃² − r²| ≤ [dp + 2(dp + 1)]·u·w(1 + O(u)) < 4(dp + 2)·u·w.
//       The clamp at TAIL_R2_MIN moves r̃² towards r² ≥ 0 or by at most TAIL_R2_MIN.  κ is TAIL_LIP-Lipschitz in r² (abo_kappa.h).
//   (b) evaluation.  |kappa_tail(r̃²) − κ(r̃²)| ≤ TAIL_ETA_EVAL (abo_kappa.h), for r̃² < 2·TAIL_W_MAX.
//       η_j = TAIL_ETA_EVAL + TAIL_LIP·(4(dp + 2)·u·w_j + TAIL_R2_MIN) bounds |κ̃ − κ| for every pair of candidate j.
//   (c) the full launch's own distance to κ: difference form (relative error (dp + 2)u of r², |r²·dκ/dr²| ≤ 0.7: 0.7(dp + 2)u), sqrt to
//       1 ulp, exp to 2 ulp (tests/test_gpu_parity.py::test_kappa_device_math), argument and polynomial roundings (together below 12u):
//       η_full = (dp + 14)·u per pair — 22u at dp = 8, 46u at dp = 32.
//   (d) summation.  Either launch adds its N products α_k·v_k (|v_k| ≤ σ_f²(1 + 2⁻⁴⁰)) in some fixed order, one rounding per product and per
//       addition, the two orders being different ones: each sum is within (Np + 16)·u·σ_f²·Σ_k|α_k| of the exact one (any order: n·u·Σ|terms|
//       to first order; the 16 cover σ_f²·α_k rounded per lane here, mean_c + head, head + tail).  Both: (2Np + 32)·u·σ_f²·‖α‖₁.
//   (e) the epilogue's μ̃ − ε rounds once more: u·|μ̃| ≤ u·(|mean_c| + 1.01·σ_f²·‖α‖₁).
//   ε_j = 1.0001·σ_f²·[(η_j + η_full)·Σ_{k ≥ R}|α_k| + (2Np + 64)·u·‖α‖₁] + 8u·|mean_c|   (1.0001: the roundings of this very expression and
//   of the two norms).  On the benchmark's problem (d = 8, unit box, ℓ = 1… w ≤ 16) η is 2⁻⁴¹ + 1.5·40u·16 ≈ 5.6·10⁻¹³.
// Non-finite input: a NaN or ±Inf coordinate gives |z|² = NaN or +Inf, hence !(w < TAIL_W_MAX), and the candidate's μ̃_tail is NaN — its
// bound is NaN and it is kept, as the head columns' non-finite check already decides.  The same test keeps the sequences of
// abo_kappa.h inside the range they are analysed for (finite coordinates beyond it: kept as well).  Within a finite candidate no pair
// can be non-finite (r̃² is clamped from below and bounded by 2w), which is why the per-pair check of kgen_rows is not needed here.
#include "kgen_core.h"

namespace abo {

template <int FAM, int DP>
__global__ void __launch_bounds__(256) kgen_tail_kernel(KgenTailArgs p) {
    __shared__ double zm[JT][DP];          // −2·z
    __shared__ double zz[JT];              // |z|²
    __shared__ double red[4][JT];
    const int t = threadIdx.x;
    const int jb = blockIdx.x * JT;
    for (int idx = t; idx < JT * DP; idx += 256) {
        const int jj = idx / DP, c = idx % DP;
        const int64_t gj = p.j0 + jb + jj;
        zm[jj][c] = (c < p.d && gj < p.M) ? -2.0 * (p.Z[gj * p.d + c] * p.s) : 0.0;
    }
    __syncthreads();
    if (t < JT) {
        double q = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) { const double z = -0.5 * zm[t][c]; q = fma(z, z, q); }
        zz[t] = q;
    }
    __syncthreads();

    double mu[JT];
#pragma unroll
    for (int jj = 0; jj < JT; ++jj) mu[jj] = 0.0;

    for (int k0 = p.k0; k0 < p.Np; k0 += KSTEP) {
        const int k = k0 + 2 * t;
        if (k < p.N) {
            // a column past the last training point reads row 0 with weight 0: neither the padding rows of Xs (which, in storage
            // shared between handles, may hold another branch's points) nor the padding of alpha are relied on
            const bool in1 = k + 1 < p.N;
            double x0[DP], x1[DP];
            const double* xp0 = p.Xs + (int64_t)k * DP;
            const double* xp1 = p.Xs + (int64_t)(in1 ? k + 1 : 0) * DP;
            if constexpr (DP >= 2) {
#pragma unroll
                for (int c = 0; c < DP; c += 2) {
                    const d2_t v0 = *reinterpret_cast<const d2_t*>(xp0 + c);
                    const d2_t v1 = *reinterpret_cast<const d2_t*>(xp1 + c);
                    x0[c] = v0[0]; x0[c + 1] = v0[1];
                    x1[c] = v1[0]; x1[c + 1] = v1[1];
                }
            } else {
                x0[0] = xp0[0]; x1[0] = xp1[0];
            }
            double xx0 = 0.0, xx1 = 0.0;
#pragma unroll
            for (int c = 0; c < DP; ++c) { xx0 = fma(x0[c], x0[c], xx0); xx1 = fma(x1[c], x1[c], xx1); }
            const double a0 = p.alpha[k] * p.sigma_f2, a1 = in1 ? p.alpha[k + 1] * p.sigma_f2 : 0.0;
#pragma unroll
            for (int jj = 0; jj < JT; ++jj) {
                asm volatile("" ::: "memory");          // keep the candidates in LDS (see kgen_rows)
                const double q = zz[jj];
                double r0 = xx0 + q, r1 = xx1 + q;
#pragma unroll
                for (int c = 0; c < DP; ++c) {
                    const double m = zm[jj][c];
                    r0 = fma(x0[c], m, r0);
                    r1 = fma(x1[c], m, r1);
                }
                mu[jj] = fma(kappa_tail<FAM>(r1), a1, fma(kappa_tail<FAM>(r0), a0, mu[jj]));
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
        const double u = 0x1p-53;
        const double a_tail = p.norms[0], a_all = p.norms[1];
        const double w = p.norms[2] + zz[t];
        const double eta = TAIL_ETA_EVAL + TAIL_LIP * (4.0 * (DP + 2) * u * w + TAIL_R2_MIN);
        const double sum = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        p.mu_tail[gj] = w < TAIL_W_MAX ? sum : __longlong_as_double(0x7ff8000000000000ll);
        p.eps[gj] = 1.0001 * p.sigma_f2 * ((eta + (DP + 14) * u) * a_tail + (2.0 * p.Np + 64.0) * u * a_all) + 8.0 * u * __builtin_fabs(p.mean_c);
    }
}

// One workgroup of 1024 threads; thread t takes the columns t, t + 1024, …, then a tree over the threads: a fixed order.
__global__ void __launch_bounds__(1024) tail_norms_kernel(const double* __restrict__ Xs, const double* __restrict__ alpha, int N, int dp,
                                                          int k0, double* __restrict__ norms) {
    __shared__ double r[3][1024];
    const int t = threadIdx.x;
    double at = 0.0, ah = 0.0, xm = 0.0;
    for (int k = t; k < N; k += 1024) {
        const double a = __builtin_fabs(alpha[k]);
        if (k >= k0) {
            at += a;
            double xx = 0.0;
            for (int c = 0; c < dp; ++c) { const double x = Xs[(int64_t)k * dp + c]; xx = fma(x, x, xx); }
            xm = xx > xm ? xx : xm;
        } else {
            ah += a;
        }
    }
    r[0][t] = at; r[1][t] = ah; r[2][t] = xm;
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if (t < o) {
            r[0][t] += r[0][t + o];
            r[1][t] += r[1][t + o];
            r[2][t] = r[2][t + o] > r[2][t] ? r[2][t + o] : r[2][t];
        }
        __syncthreads();
    }
    if (t == 0) { norms[0] = r[0][0]; norms[1] = r[0][0] + r[1][0]; norms[2] = r[2][0]; }
}

hipError_t launch_tail_norms(const double* Xs, const double* alpha, int N, int dp, int k0, double* norms, hipStream_t s) {
    if (N <= 0 || dp <= 0 || k0 < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tail_norms_kernel, dim3(1), dim3(1024), 0, s, Xs, alpha, N, dp, k0, norms);
    return hipGetLastError();
}

template <int FAM>
static hipError_t launch_tail_dp(const KgenTailArgs& a, hipStream_t s) {
    dim3 grid(a.Mc / JT), block(256);
    switch (a.dp) {
        case 1: hipLaunchKernelGGL((kgen_tail_kernel<FAM, 1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((kgen_tail_kernel<FAM, 2>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((kgen_tail_kernel<FAM, 4>), grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL((kgen_tail_kernel<FAM, 8>), grid, block, 0, s, a); break;
        case 16: hipLaunchKernelGGL((kgen_tail_kernel<FAM, 16>), grid, block, 0, s, a); break;
        case 32: hipLaunchKernelGGL((kgen_tail_kernel<FAM, 32>), grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_kgen_tail(const KgenTailArgs& a, hipStream_t s) {
    if (a.Mc <= 0) return hipSuccess;
    // whole waves of two columns per lane from an even first column; the chunk in whole workgroups
    if (a.Mc % JT || a.k0 < 0 || a.k0 % 128 || a.k0 >= a.N || a.N > a.Np) return hipErrorInvalidValue;
    switch (a.family) {
        case ABO_KERNEL_SE: return launch_tail_dp<ABO_KERNEL_SE>(a, s);
        case ABO_KERNEL_MATERN52: return launch_tail_dp<ABO_KERNEL_MATERN52>(a, s);
        case ABO_KERNEL_MATERN72: return launch_tail_dp<ABO_KERNEL_MATERN72>(a, s);
        case ABO_KERNEL_MATERN32: return launch_tail_dp<ABO_KERNEL_MATERN32>(a, s);
        default: return hipErrorInvalidValue;
    }
}

// test hook: out[i] = kappa_tail(family, d2[i])
__global__ void kappa_tail_test_kernel(int family, const double* d2, double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = d2[i];
    double v;
    if (family == ABO_KERNEL_SE) v = kappa_tail<ABO_KERNEL_SE>(x);
    else if (family == ABO_KERNEL_MATERN52) v = kappa_tail<ABO_KERNEL_MATERN52>(x);
    else if (family == ABO_KERNEL_MATERN72) v = kappa_tail<ABO_KERNEL_MATERN72>(x);
    else v = kappa_tail<ABO_KERNEL_MATERN32>(x);
    out[i] = v;
}

hipError_t launch_kappa_tail_test(int family, const double* d2, double* out, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kappa_tail_test_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, family, d2, out, n);
    return hipGetLastError();
}

}  // namespace abo
