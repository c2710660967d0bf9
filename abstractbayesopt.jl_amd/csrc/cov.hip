// Joint posterior covariance between two point sets (abo_predict_cov; api.hip drives it):
//     cov[i][j] = σ_f²·κ(‖za_i − zb_j‖/ℓ) − Σ_k V_a[i][k]·V_b[j][k],   V = K_ZX·L⁻ᵀ  (point-major rows, k over the factor rows)
// The V's and the signed product come from the fp64 MFMA GEMM family (gemm.hip: C = −A·Bᵀ + C straight onto the prior block); the
// symmetric form cov(Z_a, Z_a) takes the lower 128-tiles only and is completed by loo.hip's tile mirror.  The kernels here are the
// two ends of that chain: the prior block the product is subtracted from, and the compact copy-out of the padded result.
// No reductions and no atomics: every output element has one writer and one summation order — the same bits on every call.
#include "abo_kernels.h"
#include "abo_kappa.h"

namespace abo {

namespace {

constexpr int COV_ROWS = 16;                     // rows of the block per workgroup: four waves, four rows each

// C[i][j] = σ_f²·κ(‖As_i − Bs_j‖²) for i < Ma, j < Mb, 0 in the padding (As [⌈Ma⌉₁₂₈][dp], Bs [⌈Mb⌉₁₂₈][dp]: scaled, zero padded).
// A lane owns a column j, a wave four rows: 512-byte row stores (the mapping of dkdlogell_kernel).  The differences are formed
// directly (no x² − 2xy + y²) and summed in coordinate order: with As == Bs, e_ij = −e_ji exactly, so the block is symmetric bit for
// bit and its diagonal is exactly σ_f² (κ(0) = 1 in every family's device sequence).  sym: only the 128-tiles with tj ≤ ti are
// written — the product touches no others and the mirror fills the rest.
template <int FAM>
__global__ void __launch_bounds__(256) cov_prior_kernel(const double* __restrict__ As, const double* __restrict__ Bs, int Ma, int Mb, int dp,
                                                        double sigma_f2, int sym, double* __restrict__ C, int64_t ldc) {
    if (sym && (int)(blockIdx.x * 64) / TB > (int)(blockIdx.y * COV_ROWS) / TB) return;
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i0 = blockIdx.y * COV_ROWS + (threadIdx.x >> 6) * 4;
    const double* zb = Bs + (int64_t)j * dp;
    const double* za = As + (int64_t)i0 * dp;
    double d2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < dp; ++c) {
        const double x = zb[c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double e = za[(int64_t)r * dp + c] - x;
            d2[r] = fma(e, e, d2[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        C[(int64_t)(i0 + r) * ldc + j] = (i0 + r < Ma && j < Mb) ? sigma_f2 * kappa_eval<FAM>(d2[r]) : 0.0;
}

// out[i][j] = C[i][j] for i < Ma, j < Mb (out: compact row-major Ma × Mb); sym: + 1e-18 on the diagonal, abo_predict's latent-variance
// jitter (added here, behind the mirror, so that both triangles carry the same bits).  A lane per column: coalesced on both sides.
__global__ void __launch_bounds__(256) cov_pack_kernel(const double* __restrict__ C, int64_t ldc, int Ma, int Mb, int sym,
                                                       double* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= Mb) return;
    double v = C[(int64_t)i * ldc + j];
    if (sym && i == j) v += 1e-18;
    out[(int64_t)i * Mb + j] = v;
}

}  // namespace

hipError_t launch_cov_prior(const double* As, const double* Bs, int Ma, int Mb, int dp, int family, double sigma_f2, int sym, double* C,
                            int64_t ldc, hipStream_t s) {
    if (Ma <= 0 || Mb <= 0) return hipSuccess;
    const dim3 grid((unsigned)(pad_up(Mb, TB) / 64), (unsigned)(pad_up(Ma, TB) / COV_ROWS)), block(256);
    switch (family) {
        case ABO_KERNEL_SE: hipLaunchKernelGGL((cov_prior_kernel<ABO_KERNEL_SE>), grid, block, 0, s, As, Bs, Ma, Mb, dp, sigma_f2, sym, C, ldc); break;
        case ABO_KERNEL_MATERN52: hipLaunchKernelGGL((cov_prior_kernel<ABO_KERNEL_MATERN52>), grid, block, 0, s, As, Bs, Ma, Mb, dp, sigma_f2, sym, C, ldc); break;
        case ABO_KERNEL_MATERN72: hipLaunchKernelGGL((cov_prior_kernel<ABO_KERNEL_MATERN72>), grid, block, 0, s, As, Bs, Ma, Mb, dp, sigma_f2, sym, C, ldc); break;
        case ABO_KERNEL_MATERN32: hipLaunchKernelGGL((cov_prior_kernel<ABO_KERNEL_MATERN32>), grid, block, 0, s, As, Bs, Ma, Mb, dp, sigma_f2, sym, C, ldc); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_cov_pack(const double* C, int64_t ldc, int Ma, int Mb, int sym, double* out, hipStream_t s) {
    if (Ma <= 0 || Mb <= 0) return hipSuccess;
    hipLaunchKernelGGL(cov_pack_kernel, dim3((unsigned)((Mb + 255) / 256), (unsigned)Ma), dim3(256), 0, s, C, ldc, Ma, Mb, sym, out);
    return hipGetLastError();
}

}  // namespace abo
