// The HEAD of the FIRST bound level of the pruned top-k selection in one fused kernel (acq.hip: prune_select).
//
// A first-level bound pass over R = 256·rblocks0 rows needs, per candidate j, the head of the mean (columns k < R) and
// σ²_R = k_zz − Σ_{i<R} v_ij², V = W·K_XZ with the triangular W = L⁻¹: only the R × R head of W and the kernel values of the first R
// training points.  The int8-residue pipeline (head generator with eight residue planes, residue GEMM, reconstruction) pays its fixed
// costs and 270 MB of planes per chunk for that.  Here one workgroup takes 64 candidates and
//   * generates their R kernel values in fp64 with the generator's per-pair arithmetic (kgen_core.h: difference form, fma chain,
//     kappa_eval, times σ_f²) — a lane is a candidate, a wave walks every fourth training point (uniform operands), so the head of the
//     mean is one fp64 fma chain per lane and a serial sum over the four waves: fixed order, no atomics;
//   * keeps K̂ = fl32(those values) in LDS (256 × 64 floats) and multiplies by Ŵ = fl32(W) on the fp32 matrix pipe
//     (v_mfma_f32_32x32x2_f32: exact fp32 products, an fp32 fma chain over k); wave w owns the 32-row blocks w and 7 − w of a 256-row
//     group — 9 k-blocks each on the diagonal group, the triangle's zero blocks are skipped;
//   * closes with S̃_j = (1 − c)·Σ_i max(|Ṽ_ij| − δ_i, 0)² in fp64 (the accumulator's column is the lane, its rows the registers).
// R > 256: the row groups in turn, each against the k-groups up to its own (kernel values of an earlier k-group are generated again;
// the head of the mean is summed on the diagonal groups alone).
// head32_prep_kernel writes Ŵ in the MFMA's A-fragment order (a wave reads 1 KB contiguous per 8 columns), ‖W_i‖₁ and δ_i — per bound
// pass, like oz_prepare_w_bound: nothing cached, nothing to invalidate.
//
// The guard.  v = 2⁻²⁴, u = 2⁻⁵³, τ = 2⁻¹²⁶, n = i + 1, L_i = ‖W_i‖₁ (the kernel uses L1u = L1·(1 + n·2⁻⁵²) ≥ L_i of its own fp64 sum),
// kmax = σ_f²(1 + 2⁻⁴⁰) ≥ every fp64 kernel value either pass computes, v_ij the FULL pass's computed value.  δ_i ≥ |Ṽ_ij − v_ij|:
//   (1) ŵ = fl32(w): |ŵ − w| ≤ v|w| + τ (τ: an entry below the normal range, flushed or not);
//   (2) k̂ = fl32(k): |k̂ − k| ≤ v·k + τ.  k is this kernel's fp64 value; the full pass's generator runs the same source per pair, but
//       nothing here relies on equal bits: both are within η_full·σ_f² of σ_f²·κ, η_full = (dp + 14)·u (kgen_tail.hip (c)), so the two
//       differ by at most 2η_full·σ_f² per entry.
//       (1), (2) and the full pass's other operand: |Σ ŵk̂ − Σ w·k_full| ≤ L·kmax·(2v + v² + 2η_full) + τ·(2n·kmax + 2L + n);
//   (3) the fp32 dot product of n non-zero terms (ŵ_ik = 0 exactly for k > i; adding 0 is exact) in ANY association order, with or
//       without fused multiply-add: ≤ γ_{n+1}·Σ|ŵ||k̂| ≤ γ_{R+1}·(1 + v)²·L·kmax, γ_m = m·v/(1 − m·v);
//   (4) range.  A row with L, kmax or L·kmax ≥ 2¹⁰⁰, or a non-finite entry, is FLAGGED: Ŵ_i = 0, δ_i = +∞, it contributes 0 (no
//       row scale: such rows do not occur in a factor that is of any use).  Otherwise no product or partial sum leaves the fp32
//       range.  Denormals: the guide says the MFMA keeps them in C/D and treats A/B as the VALU does; nothing here depends on
//       it — with EVERY denormal input, product and partial sum flushed, each of the n products and n sums loses at most τ: 2n·τ.
//       This is an assumption-free cover, not a measurement;
//   (5) the full pass's v_ij against the real product of its fp64 operands.  int8 engine (ozaki.hip, "the guarded bound"):
//       A(s'', sK'') + rec_full·2^−(s''+sK''), with 2^−s'' = max(2^(e1+53−eP), 2^(e2−52)) ≤ L·(2⁻⁵¹ + 2^(54−eP)) =: T (L < 2^e1 ≤ 2L,
//       max|w| < 2^e2 ≤ 2L), so A ≤ ½·2^−sK''·L + ½·T·n·kmax + ¼·n·T·2^−sK''; fp64 GEMM: γ⁶⁴_n·L·kmax ≤ 2n·u·L·kmax.  δ takes the sum
//       of both, and 2⁻⁵⁰·L·kmax for the closing roundings of either;
//   δ_i = (1 + 2⁻³⁰)·[(1) + … + (5)] (the factor: the roundings of this expression, all terms positive, fewer than 64 operations).
//   At C3 (R = 256, σ_f² = 1): δ_i = ‖W_i‖₁·(2 + 257 + …)·2⁻²⁴ = ‖W_i‖₁·1.55·10⁻⁵.
// Then t_ij = max(|Ṽ_ij| − δ_i, 0) ≤ |v_ij|; formed in fp64 (the conversion is exact) it carries one rounding, its square and the sum
// of R of them R + 1 more, the sum over lanes and waves 8 more: computed ≤ (1 + u)^(R + 12)·Σt².  The full pass's fp64 sum of squares
// over all Np rows in its order is ≥ (1 − u)^(Np + 2) of the exact sum of its computed v², every term being non-negative, hence of the
// first R terms.  c = (Np + R + 64)·2⁻⁵² makes S̃ = (1 − c)·Σt² ≤ the full pass's COMPUTED column sum, as a number.
// Non-finite input: a candidate with a non-finite kernel value anywhere in its head (a NaN or infinite coordinate) gets S̃ = NaN,
// so does a non-finite sum; the bound is then NaN and the candidate is kept — the tail's μ̃ = NaN says the same.
#include "kgen_core.h"

namespace abo {

constexpr int H32_JT = 64;       // candidates per workgroup
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef float f16_t __attribute__((ext_vector_type(16)));

// one wave per row of the head: L1 norm, flag, δ, and the row's part of Ŵ in fragment order —
// Wf[((ib·(R/8) + g)·64 + lane)·4 + e] = fl32(W[32·ib + (lane & 31)][8g + 2e + (lane >> 5)]) for g < 4(ib + 1), zero above the diagonal
__global__ void __launch_bounds__(256) head32_prep_kernel(KgenHead32Args p) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= p.R) return;
    const double* w = p.W + (int64_t)row * p.ldw;
    double l1 = 0.0;
    for (int k = lane; k <= row; k += 64) l1 += __builtin_fabs(w[k]);
#pragma unroll
    for (int o = 32; o; o >>= 1) l1 += __shfl_xor(l1, o);
    const double kmax = p.sigma_f2 * (1.0 + 0x1p-40);
    const bool ok = l1 < 0x1p100 && kmax < 0x1p100 && l1 * kmax < 0x1p100;          // (a NaN fails every comparison)
    const int ib = row >> 5, ir = row & 31, kend = 32 * (ib + 1);
    float* wf = p.Wf + (int64_t)ib * (p.R / 8) * 256;
    for (int k = lane; k < kend; k += 64) {
        const float x = (ok && k <= row) ? (float)w[k] : 0.0f;
        wf[((k >> 3) * 64 + ((k & 1) << 5) + ir) * 4 + ((k >> 1) & 3)] = x;
    }
    if (lane == 0) {
        double dl = __builtin_inf();
        if (ok) {
            const double v = 0x1p-24, u = 0x1p-53, tau = 0x1p-126;
            const double n = (double)(row + 1);
            const double L = l1 * (1.0 + n * 0x1p-52);
            const double g = (p.R + 1.0) * v / (1.0 - (p.R + 1.0) * v);
            const double T = L * (0x1p-51 + __builtin_ldexp(1.0, 54 - p.eP_full));
            const double sk = __builtin_ldexp(1.0, -p.sK_full);
            const double full = 0.5 * sk * L + 0.5 * T * n * kmax + 0.25 * n * T * sk + p.rec_full * T * sk + 2.0 * n * u * L * kmax + 0x1p-50 * L * kmax;
            dl = L * kmax * (2.0 * v + v * v + 2.0 * (p.dp + 14) * u + g * (1.0 + v) * (1.0 + v)) + tau * (2.0 * n * kmax + 2.0 * L + 3.0 * n) + full;
            dl *= 1.0 + 0x1p-30;
        }
        p.delta[row] = dl;
        p.l1[row] = l1;
    }
}

// the two accumulators (candidate columns 0-31 and 32-63) of one 32-row block against the k-steps [0, 8·ng) of the LDS block
__device__ __forceinline__ void head32_rowblock(const float* __restrict__ wf, const float (*ks)[H32_JT], int ng, int lane, f16_t& c0, f16_t& c1) {
    const int h = lane >> 5, jl = lane & 31;
    const int col0 = jl ^ (h << 5), col1 = col0 ^ 32;          // odd k rows are stored with the column halves swapped (bank spread)
    const f4_t* ap = reinterpret_cast<const f4_t*>(wf) + lane;
    f4_t a = ap[0];
    for (int g = 0; g < ng; ++g) {
        const f4_t an = ap[(g + 1 < ng ? g + 1 : g) * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = 8 * g + 2 * e + h;
            const float b0 = ks[k][col0], b1 = ks[k][col1];
            c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b0, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b1, c1, 0, 0, 0);
        }
        a = an;
    }
}

// Σ over the block's 16 rows of this lane of max(|c| − δ, 0)², rows in register order
__device__ __forceinline__ double head32_squares(const f16_t& c, const double* __restrict__ delta, int row0, int h, double s) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const double dl = delta[row0 + 8 * (r >> 2) + 4 * h + (r & 3)];
        double t = __builtin_fabs((double)c[r]) - dl;
        t = t > 0.0 ? t : 0.0;
        s = fma(t, t, s);
    }
    return s;
}

template <int FAM, int DP>
__global__ void __launch_bounds__(256) kgen_head32_kernel(KgenHead32Args p) {
    __shared__ __attribute__((aligned(16))) float ks[256][H32_JT];
    __shared__ double mred[4][H32_JT];
    __shared__ double sred[8][H32_JT];
    __shared__ int bred[4][H32_JT];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t gj = (int64_t)blockIdx.x * H32_JT + lane;
    double z[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) z[c] = (c < p.d && gj < p.M) ? p.Z[gj * p.d + c] * p.s : 0.0;

    double mu = 0.0, ssq0 = 0.0, ssq1 = 0.0;
    int bad = 0;
    const int h = lane >> 5;
    const int ngroups = p.R / 256;
    for (int rg = 0; rg < ngroups; ++rg) {
        f16_t acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
        const int ibA = rg * 8 + wave, ibB = rg * 8 + 7 - wave;          // global 32-row blocks of this wave
        for (int kg = 0; kg <= rg; ++kg) {
            if (rg + kg) __syncthreads();                                // the block before has been read
            // kernel values of the k-group: the generator's arithmetic per pair, one candidate per lane
            const bool diag = kg == rg;
            const int swz = (wave & 1) << 5;
#pragma unroll 4
            for (int m = 0; m < 64; ++m) {
                const int kl = wave + 4 * m, k = kg * 256 + kl;          // (k < R ≤ N: no padding row is read)
                const double* xp = p.Xs + (int64_t)k * DP;
                double r = 0.0;
#pragma unroll
                for (int c = 0; c < DP; ++c) {
                    const double e = xp[c] - z[c];
                    r = fma(e, e, r);
                }
                const double v = p.sigma_f2 * kappa_eval<FAM>(r);
                if (!(__builtin_fabs(v) < 1.0e300)) bad = 1;
                if (diag) mu = fma(v, p.alpha[k], mu);
                ks[kl][lane ^ swz] = (float)v;
            }
            __syncthreads();
            const int ng = diag ? 4 : 32;
            head32_rowblock(p.Wf + ((int64_t)ibA * (p.R / 8) + kg * 32) * 256, ks, diag ? ng * (wave + 1) : ng, lane, acc[0], acc[1]);
            head32_rowblock(p.Wf + ((int64_t)ibB * (p.R / 8) + kg * 32) * 256, ks, diag ? ng * (8 - wave) : ng, lane, acc[2], acc[3]);
        }
        ssq0 = head32_squares(acc[0], p.delta, ibA * 32, h, ssq0);
        ssq1 = head32_squares(acc[1], p.delta, ibA * 32, h, ssq1);
        ssq0 = head32_squares(acc[2], p.delta, ibB * 32, h, ssq0);
        ssq1 = head32_squares(acc[3], p.delta, ibB * 32, h, ssq1);
    }
    // fixed-order reductions: 4 waves (mean, flags), 4 waves × 2 lane halves (squares)
    mred[wave][lane] = mu;
    bred[wave][lane] = bad;
    sred[wave * 2 + h][lane & 31] = ssq0;
    sred[wave * 2 + h][32 + (lane & 31)] = ssq1;
    __syncthreads();
    if (t < H32_JT && gj < p.M) {
        p.head[gj] = p.mean_c + (((mred[0][t] + mred[1][t]) + mred[2][t]) + mred[3][t]);
        double s = sred[0][t];
#pragma unroll
        for (int q = 1; q < 8; ++q) s += sred[q][t];
        s *= 1.0 - (p.Np + p.R + 64.0) * 0x1p-52;
        const bool b = (bred[0][t] | bred[1][t] | bred[2][t] | bred[3][t]) != 0;
        p.ssq[gj] = (!b && s < __builtin_inf()) ? s : __longlong_as_double(0x7ff8000000000000ll);
    }
}

template <int FAM>
static hipError_t launch_head32_dp(const KgenHead32Args& a, hipStream_t s) {
    dim3 grid((unsigned)((a.M + H32_JT - 1) / H32_JT)), block(256);
    switch (a.dp) {
        case 1: hipLaunchKernelGGL((kgen_head32_kernel<FAM, 1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((kgen_head32_kernel<FAM, 2>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((kgen_head32_kernel<FAM, 4>), grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL((kgen_head32_kernel<FAM, 8>), grid, block, 0, s, a); break;
        case 16: hipLaunchKernelGGL((kgen_head32_kernel<FAM, 16>), grid, block, 0, s, a); break;
        case 32: hipLaunchKernelGGL((kgen_head32_kernel<FAM, 32>), grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_kgen_head32(const KgenHead32Args& a, hipStream_t s) {
    if (a.M <= 0) return hipSuccess;
    // whole 256-row groups, all of them real training points (no padding row of Xs, alpha or W is read), γ_{R+1} far below 1
    if (a.R <= 0 || a.R % 256 || a.R > a.N || a.R > 2048 || a.N > a.Np || a.d > a.dp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(head32_prep_kernel, dim3(a.R / 4), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    switch (a.family) {
        case ABO_KERNEL_SE: return launch_head32_dp<ABO_KERNEL_SE>(a, s);
        case ABO_KERNEL_MATERN52: return launch_head32_dp<ABO_KERNEL_MATERN52>(a, s);
        case ABO_KERNEL_MATERN72: return launch_head32_dp<ABO_KERNEL_MATERN72>(a, s);
        case ABO_KERNEL_MATERN32: return launch_head32_dp<ABO_KERNEL_MATERN32>(a, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace abo
