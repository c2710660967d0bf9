// The cross-kernel generator of a VALUE-ONLY model against derivative query outputs (abo_predict_deriv): the rows
// (f(z_j), ∂f(z_j)/∂z_1 … ∂f(z_j)/∂z_d) of a chunk of query points against the N function values the model is conditioned on, and their
// products with alpha.  With e = (x_k − z_j)/ℓ, u = ‖e‖² and k = σ_f²φ(u) (the header comment of kgen_grad_core.h, taken for a value
// training row):
//     Kout[j·p + 0][k]     = cov(f(z_j), f(x_k))         =  σ_f²·φ(u)
//     Kout[j·p + c + 1][k] = cov(∂f(z_j)/∂z_c, f(x_k))   = −σ_f²·φ'(u)·2e_c/ℓ
// One lane per (query point, training point) pair: u, φ and φ' are computed once and fanned out to the point's p = d + 1 rows; the
// lanes of a wave hold consecutive training points, so every row store of a wave is one contiguous 512-byte run.  The lane's training
// point stays in registers over the workgroup's PJ query points, whose scaled coordinates are staged in LDS (broadcast reads).
// PJ·(DP + 1) ≤ 36 mean accumulators per lane: PJ = 4 points up to dp = 8, 2 at dp = 16, 1 at dp = 32.
// mu_rows: each lane sums its training points k = t, t + 256, … in that order, then the xor tree over the 64 lanes, then the four
// waves in order — no atomics, the same bits on every launch, and independent of how the points are cut into chunks.
// kgen_grad_kernel serves the same rows for pt = 1 only formally (its lanes carry the state of derivative TRAINING rows — the second
// coordinate difference, φ'' — and evaluate φ once per row instead of once per point).
#include "kgen_grad_core.h"

namespace abo {

namespace {

constexpr int ZROWS = 16;     // padding rows zeroed by one of the extra workgroups

template <int DP> constexpr int deriv_pj() { return DP <= 8 ? 4 : (DP == 16 ? 2 : 1); }

template <int FAM, int DP>
__global__ void __launch_bounds__(256) kgen_deriv_kernel(KgenDerivArgs p) {
    constexpr int PJ = deriv_pj<DP>();
    constexpr int PMAX = DP + 1;
    __shared__ double zs[PJ][DP];
    __shared__ double red[4][PJ * PMAX];
    const int t = threadIdx.x;
    const int pr = p.d + 1;                                        // rows per point
    const int nwg = (p.npts + PJ - 1) / PJ;                        // workgroups that hold points; the rest zero the padding rows
    if ((int)blockIdx.x >= nwg) {
        const int64_t r0 = (int64_t)p.npts * pr + (int64_t)((int)blockIdx.x - nwg) * ZROWS;
        const int64_t r1 = r0 + ZROWS < p.rows_pad ? r0 + ZROWS : p.rows_pad;
        for (int64_t r = r0; r < r1; ++r) {
            for (int k = t; k < p.Np; k += 256) p.Kout[r * p.ldk + k] = 0.0;
            if (p.mu_rows && t == 0) p.mu_rows[r] = 0.0;
        }
        return;
    }
    const int jb = blockIdx.x * PJ;                                // first point of the workgroup, relative to the chunk
    for (int idx = t; idx < PJ * DP; idx += 256) {
        const int jj = idx / DP, c = idx % DP;
        zs[jj][c] = (c < p.d && jb + jj < p.npts) ? p.Z[(p.pt0 + jb + jj) * p.d + c] * p.s : 0.0;
    }
    __syncthreads();
    const double cg = -2.0 * p.s * p.sigma_f2;                     // a derivative row: cg·φ'(u)·e_c
    double mu[PJ][PMAX];
#pragma unroll
    for (int jj = 0; jj < PJ; ++jj)
#pragma unroll
        for (int q = 0; q < PMAX; ++q) mu[jj][q] = 0.0;

    for (int k = t; k < p.Np; k += 256) {                          // (Np is a multiple of 128: whole waves)
        double x[DP];
        const double* xp = p.Xs + (int64_t)k * DP;
        if constexpr (DP >= 2) {
#pragma unroll
            for (int c = 0; c < DP; c += 2) {
                const d2_t v = *reinterpret_cast<const d2_t*>(xp + c);
                x[c] = v[0]; x[c + 1] = v[1];
            }
        } else {
            x[0] = xp[0];
        }
        const bool okk = k < p.N;
        const double a = (okk && p.alpha) ? p.alpha[k] : 0.0;
#pragma unroll
        for (int jj = 0; jj < PJ; ++jj) {
            if (jb + jj >= p.npts) break;                          // workgroup-uniform
            // keep the query coordinates in LDS (kgen_core.h: hipcc would hoist them out of the sweep into registers)
            asm volatile("" ::: "memory");
            double e[DP];
            double u = 0.0;
#pragma unroll
            for (int c = 0; c < DP; ++c) {
                e[c] = x[c] - zs[jj][c];
                u = fma(e[c], e[c], u);
            }
            double f0, f1, f2;
            phi_derivs<FAM>(u, f0, f1, f2);
            double* row = p.Kout + ((int64_t)(jb + jj) * pr) * p.ldk + k;
            const double v0 = okk ? p.sigma_f2 * f0 : 0.0;
            row[0] = v0;
            mu[jj][0] = fma(v0, a, mu[jj][0]);
            const double g = cg * f1;
#pragma unroll
            for (int c = 0; c < DP; ++c) {
                if (c < p.d) {                                     // uniform
                    const double v = okk ? g * e[c] : 0.0;
                    row[(int64_t)(c + 1) * p.ldk] = v;
                    mu[jj][c + 1] = fma(v, a, mu[jj][c + 1]);
                }
            }
        }
    }
    if (p.mu_rows == nullptr) return;
    // fixed-order reduction: lanes (xor tree) → 4 waves (serial)
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int jj = 0; jj < PJ; ++jj)
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            double v = mu[jj][q];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) red[wave][jj * PMAX + q] = v;
        }
    __syncthreads();
    if (t < PJ * PMAX) {
        const int jj = t / PMAX, q = t % PMAX;
        if (jb + jj < p.npts && q < pr)
            p.mu_rows[(int64_t)(jb + jj) * pr + q] = (q == 0 ? p.mean_c : 0.0) + (((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]);
    }
}

template <int FAM, int DP>
hipError_t launch_dp(const KgenDerivArgs& a, hipStream_t s) {
    constexpr int PJ = deriv_pj<DP>();
    const int64_t pad = a.rows_pad - (int64_t)a.npts * (a.d + 1);
    const unsigned grid = (unsigned)((a.npts + PJ - 1) / PJ + (pad + ZROWS - 1) / ZROWS);
    hipLaunchKernelGGL((kgen_deriv_kernel<FAM, DP>), dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int FAM>
hipError_t launch_fam(const KgenDerivArgs& a, hipStream_t s) {
    switch (a.dp) {
        case 1: return launch_dp<FAM, 1>(a, s);
        case 2: return launch_dp<FAM, 2>(a, s);
        case 4: return launch_dp<FAM, 4>(a, s);
        case 8: return launch_dp<FAM, 8>(a, s);
        case 16: return launch_dp<FAM, 16>(a, s);
        case 32: return launch_dp<FAM, 32>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_kgen_deriv(const KgenDerivArgs& a, hipStream_t s) {
    if (!a.Xs || !a.Z || !a.Kout) return hipErrorInvalidValue;
    if (a.d < 1 || a.d > 32 || a.dp < a.d || a.dp > 32) return hipErrorInvalidValue;
    if (a.Np <= 0 || a.Np % TB || a.N < 0 || a.N > a.Np || a.ldk < a.Np) return hipErrorInvalidValue;
    if (a.npts < 0 || a.pt0 < 0 || a.pt0 + a.npts > a.M || a.rows_pad < (int64_t)a.npts * (a.d + 1)) return hipErrorInvalidValue;
    if (a.family != ABO_KERNEL_SE && a.family != ABO_KERNEL_MATERN52 && a.family != ABO_KERNEL_MATERN72) return hipErrorInvalidValue;
    if (a.dp & (a.dp - 1)) return hipErrorInvalidValue;            // 1, 2, 4, 8, 16, 32
    if (a.rows_pad == 0) return hipSuccess;
    switch (a.family) {
        case ABO_KERNEL_SE: return launch_fam<ABO_KERNEL_SE>(a, s);
        case ABO_KERNEL_MATERN52: return launch_fam<ABO_KERNEL_MATERN52>(a, s);
        default: return launch_fam<ABO_KERNEL_MATERN72>(a, s);
    }
}

}  // namespace abo
