// Blocked bordered append (abo_append_batch; api.hip drives it): condition a view of N points on k ≤ 64 more in one step.
//     B = W·K_b,   S = K_bb + noise·I − BᵀB = L_s·L_sᵀ,   C = Wᵀ·B,   r = δ_b − K_bᵀα,   β = S⁻¹r
//     L' = [[L, 0], [Bᵀ, L_s]]     W' = [[W, 0], [−L_s⁻¹Cᵀ, L_s⁻¹]]     α' = [α − Cβ ; β]
// The launches of a step, in order (each tri_skinny is two: the slices, then their ordered sum):
//   points     the k new rows of Xraw / Xs / ybuf / delta, *info = 0
//   newcols    K_b (N × kp) and K_bb (k × kp) behind it, kp = k padded to 16, zero in the padding columns
//   tri_skinny B = tril(W)·K_b       ┐  the two block products on v_mfma_f64_16x16x4_f64: each streams one triangle once, whatever k
//   gram       BᵀB and K_bᵀα in G partial sums
//   small      one workgroup: S, its Cholesky with the pivot check, L_s⁻¹, r, β, the log-det and quad increments
//   tri_skinny C = triu(WT)·B        ┘
//   write      rows N … N+k−1 of L and W, the matching columns of WT, α'
// Reproducible: every sum has one writer and one order — the inner dimension of a block product is cut into TS_SLICES fixed slices
// whose partial sums a second launch adds in slice order, the G partial Gram sums are added in block order.  No atomics.
#include "abo_kernels.h"
#include "abo_kappa.h"

namespace abo {

namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));

// ---- the new points ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ab_points_kernel(const double* __restrict__ Xb, const double* __restrict__ yb, int k, int d, int dp,
                                                        double s, double mean_c, double* __restrict__ Xraw_rows,
                                                        double* __restrict__ Xs_rows, double* __restrict__ y_at,
                                                        double* __restrict__ delta_at, int64_t* info) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) *info = 0;
    if (idx < k * dp) {
        const int i = idx / dp, c = idx - i * dp;
        double v = 0.0;
        if (c < d) {
            v = Xb[(int64_t)i * d + c];
            Xraw_rows[(int64_t)i * d + c] = v;
        }
        Xs_rows[idx] = c < d ? v * s : 0.0;
    }
    if (idx < k) {
        const double y = yb[idx];
        y_at[idx] = y;
        delta_at[idx] = y - mean_c;
    }
}

// Kb[j][i] = σ_f²·κ(‖xs_i − x_j·s‖²) for the training rows j < N and, behind them, the k × k block of the new points among themselves
// (rows N + jj), with cand_newcol_kernel's arithmetic — what k sequential appends and the refit's generator evaluate.  The block is
// symmetric bit for bit (the pair is always taken as (larger index, smaller index), the order a sequential append sees it in) and σ_f²
// on its diagonal.  Columns k ≤ i < kp are zero.  Xs_new: the scaled new points [k][dp]; Xraw: [N + k][d].
template <int FAM>
__global__ void __launch_bounds__(256) ab_newcols_kernel(const double* __restrict__ Xs_new, const double* __restrict__ Xraw,
                                                         double* __restrict__ Kb, int N, int k, int kp, int d, int dp, double s,
                                                         double sigma_f2) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)(N + k) * kp) return;
    const int j = (int)(idx / kp), i = (int)(idx - (int64_t)j * kp);
    double v = 0.0;
    if (i < k) {
        int a = i, b = j;
        if (j >= N) {
            const int jj = j - N;
            a = jj > i ? jj : i;
            b = N + (jj > i ? i : jj);
        }
        if (j >= N && j - N == i) {
            v = sigma_f2;
        } else {
            const double* x = Xs_new + (int64_t)a * dp;
            const double* z = Xraw + (int64_t)b * d;
            double r = 0.0;
            for (int c = 0; c < d; ++c) {
                const double e = x[c] - z[c] * s;
                r = fma(e, e, r);
            }
            v = sigma_f2 * kappa_eval<FAM>(r);
        }
    }
    Kb[idx] = v;
}

// ---- the skinny triangular product -------------------------------------------------------------------------------------------------
// out[N × kp] = tri(Wm)·V, V [N][kp] row-major, kp = 16·NB ≤ 64; lower = 1: k ≤ r, 0: r ≤ k < N.  Only rows and columns < N of Wm
// are used: what lies beyond (the remains of a discarded branch) is masked to zero in both operands before it reaches the matrix pipe.
// A workgroup takes a strip of 128 rows and one of TS_SLICES slices of the inner dimension; each of its four waves owns 32 rows (two
// 16-row tiles that share every fragment of V) and walks the part of the slice its rows' triangle covers, 16 columns a step.  The
// instruction sums over four k per issue and does not care which: lane (i = l & 15, g = l >> 4) feeds it k = k0 + 4g + t in step t,
// so that a lane reads 32 contiguous bytes of its row of Wm and the four lane groups together 128 — full-width row segments, each byte
// of the triangle read once, streamed past the caches.  V's fragments come through L2 (N·kp·8 bytes, re-read by every strip).
// D map of v_mfma_f64_16x16x4_f64: lane l, reg r → row (l >> 4) + 4r, column l & 15.
// At k = 64 a wave issues 32 MFMAs per 4 KiB of Wm: the arithmetic is then as long as the stream.  Measured: flat in k
// up to 16 at a third of trmv_kernel's bandwidth — two 32-byte loads of Wm in flight per lane and step leave it latency-bound.
constexpr int TS_ROWS = 128;      // rows of a strip (workgroup)
constexpr int TS_WROWS = 32;      // rows of a wave
constexpr int TS_SLICES = 8;      // fixed: the partial sums are added in slice order by ts_reduce_kernel

// the inner range [kb, ke) that the 32-row group `grp` shares with slice sl (empty: kb >= ke); both ends multiples of 16 or N
__host__ __device__ inline void ts_range(int N, int grp, int sl, int lower, int* kb, int* ke) {
    const int ks = ((N + TS_SLICES - 1) / TS_SLICES + 15) / 16 * 16;
    const int r0 = grp * TS_WROWS;
    int b = lower ? 0 : r0;
    int e = lower ? (r0 + TS_WROWS < N ? r0 + TS_WROWS : N) : N;
    if (b < sl * ks) b = sl * ks;
    if (e > (sl + 1) * ks) e = (sl + 1) * ks;
    *kb = b;
    *ke = e;
}

template <int NB>
__global__ void __launch_bounds__(256) ts_product_kernel(const double* __restrict__ Wm, int64_t ld, const double* __restrict__ V,
                                                         double* __restrict__ part, int N, int lower) {
    constexpr int kp = 16 * NB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int grp = blockIdx.x * (TS_ROWS / TS_WROWS) + wave;
    const int row0 = grp * TS_WROWS;
    if (row0 >= N) return;
    int kb, ke;
    ts_range(N, grp, blockIdx.y, lower, &kb, &ke);
    if (kb >= ke) return;                                   // (ts_reduce_kernel skips the same pairs)
    const int ra = row0 + r16, rb = row0 + 16 + r16;        // this lane's rows of the two tiles
    const double* pa = Wm + (int64_t)(ra < N ? ra : N - 1) * ld + 4 * g;
    const double* pb = Wm + (int64_t)(rb < N ? rb : N - 1) * ld + 4 * g;
    d4_t acc[2][NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { acc[0][nb] = d4_t{0.0, 0.0, 0.0, 0.0}; acc[1][nb] = d4_t{0.0, 0.0, 0.0, 0.0}; }
#pragma unroll 2
    for (int k0 = kb; k0 < ke; k0 += 16) {
        d4_t a = __builtin_nontemporal_load(reinterpret_cast<const d4_t*>(pa + k0));    // ld ≥ N padded to 16: inside the row
        d4_t b = __builtin_nontemporal_load(reinterpret_cast<const d4_t*>(pb + k0));
        double v[4][NB];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kk = k0 + 4 * g + t;
            const bool in = kk < N;
            const bool ua = in && ra < N && (lower ? kk <= ra : kk >= ra);
            const bool ub = in && rb < N && (lower ? kk <= rb : kk >= rb);
            a[t] = ua ? a[t] : 0.0;
            b[t] = ub ? b[t] : 0.0;
            const double* vr = V + (int64_t)(in ? kk : N - 1) * kp + r16;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const double x = vr[16 * nb];
                v[t][nb] = in ? x : 0.0;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                acc[0][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], v[t][nb], acc[0][nb], 0, 0, 0);
                acc[1][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[t], v[t][nb], acc[1][nb], 0, 0, 0);
            }
    }
    double* po = part + (int64_t)blockIdx.y * N * kp;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 16 * rt + g + 4 * r;
            if (row < N) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) po[(int64_t)row * kp + 16 * nb + r16] = acc[rt][nb][r];
            }
        }
}

// out[r][c] = the partial sums of the slices that row r's group shares the triangle with, in slice order
__global__ void __launch_bounds__(256) ts_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int N, int kp, int lower) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * kp) return;
    const int grp = (int)(idx / kp) / TS_WROWS;
    double acc = 0.0;
    for (int sl = 0; sl < TS_SLICES; ++sl) {
        int kb, ke;
        ts_range(N, grp, sl, lower, &kb, &ke);
        if (kb < ke) acc += part[(int64_t)sl * N * kp + idx];
    }
    out[idx] = acc;
}

// ---- BᵀB and K_bᵀα -----------------------------------------------------------------------------------------------------------------
// Block g sums its rows [g·rpb, (g + 1)·rpb) ∩ [0, N) in row order, 64 rows at a time through LDS: gpart[g] = {kp·kp sums of
// B[r][i]·B[r][j], kp sums of Kb[r][i]·α[r]}.  Thread t owns the entries t, t + 256, … of the kp × kp block.
constexpr int GRAM_CHUNK = 64;
template <int NB>
__global__ void __launch_bounds__(256) ab_gram_kernel(const double* __restrict__ Bm, const double* __restrict__ Kb,
                                                      const double* __restrict__ alpha, int N, int rpb, double* __restrict__ gpart) {
    constexpr int kp = 16 * NB, nper = NB * NB;
    __shared__ double sB[GRAM_CHUNK][kp + 1];
    const int t = threadIdx.x;
    const int r_lo = blockIdx.x * rpb, r_hi = r_lo + rpb < N ? r_lo + rpb : N;
    double acc[nper];
#pragma unroll
    for (int m = 0; m < nper; ++m) acc[m] = 0.0;
    double ka = 0.0;
    for (int c0 = r_lo; c0 < r_hi; c0 += GRAM_CHUNK) {
        const int nr = r_hi - c0 < GRAM_CHUNK ? r_hi - c0 : GRAM_CHUNK;
        __syncthreads();
        for (int e = t; e < GRAM_CHUNK * kp; e += 256) {
            const int r = e / kp, c = e - r * kp;
            sB[r][c] = r < nr ? Bm[(int64_t)(c0 + r) * kp + c] : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int r = 0; r < GRAM_CHUNK; ++r) {
#pragma unroll
            for (int m = 0; m < nper; ++m) {
                const int e = t + 256 * m, i = e / kp, j = e - i * kp;       // (kp a compile-time power of two or 48: shifts)
                acc[m] = fma(sB[r][i], sB[r][j], acc[m]);
            }
        }
        if (t < kp)
            for (int r = 0; r < nr; ++r) ka = fma(Kb[(int64_t)(c0 + r) * kp + t], alpha[c0 + r], ka);
    }
    double* o = gpart + (int64_t)blockIdx.x * (kp * kp + kp);
#pragma unroll
    for (int m = 0; m < nper; ++m) o[t + 256 * m] = acc[m];
    if (t < kp) o[kp * kp + t] = ka;
}

// ---- the k × k part, one workgroup -------------------------------------------------------------------------------------------------
// S = K_bb + noise·I − Σ_g gram[g] (block order), right-looking Cholesky in LDS; a pivot that is not positive at row j ends the step:
// *info = N + j + 1 (the order a refit's potrf reports), nothing else written.  Otherwise sm = {L_s [kp][kp] (lower, zero above),
// L_s⁻¹ [kp][kp] (lower), β [kp]}, scal = {2·Σ log diag L_s, ‖L_s⁻¹r‖²}.
constexpr int AB_LDS = APPEND_BATCH_MAX + 1;
__global__ void __launch_bounds__(256) ab_small_kernel(const double* __restrict__ Kbb, const double* __restrict__ gpart, int G,
                                                       const double* __restrict__ delta_b, int N, int k, int kp, double noise,
                                                       double* __restrict__ sm, double* __restrict__ scal, int64_t* info) {
    __shared__ double S[APPEND_BATCH_MAX][AB_LDS], Li[APPEND_BATCH_MAX][AB_LDS];
    __shared__ double rv[APPEND_BATCH_MAX], uv[APPEND_BATCH_MAX];
    __shared__ int bad;
    const int t = threadIdx.x;
    const int gstride = kp * kp + kp;
    if (t == 0) bad = -1;
    for (int e = t; e < k * k; e += 256) {
        const int i = e / k, j = e - i * k;
        double g = 0.0;
        for (int b = 0; b < G; ++b) g += gpart[(int64_t)b * gstride + i * kp + j];
        S[i][j] = Kbb[i * kp + j] + (i == j ? noise : 0.0) - g;
        Li[i][j] = 0.0;
    }
    if (t < k) {
        double g = 0.0;
        for (int b = 0; b < G; ++b) g += gpart[(int64_t)b * gstride + kp * kp + t];
        rv[t] = delta_b[t] - g;
    }
    __syncthreads();
    for (int j = 0; j < k; ++j) {
        if (t == 0) {
            const double p = S[j][j];
            if (!(p > 0.0)) bad = j;
            else S[j][j] = sqrt(p);
        }
        __syncthreads();
        if (bad >= 0) {
            if (t == 0 && *info == 0) *info = (int64_t)N + bad + 1;
            return;
        }
        const double piv = S[j][j];
        for (int i = j + 1 + t; i < k; i += 256) S[i][j] /= piv;
        __syncthreads();
        const int m = k - j - 1;                            // trailing block, lower triangle: (i, c), j < c ≤ i
        for (int e = t; e < m * m; e += 256) {
            const int i = j + 1 + e / m, c = j + 1 + e % m;
            if (c <= i) S[i][c] = fma(-S[i][j], S[c][j], S[i][c]);
        }
        __syncthreads();
    }
    if (t < k) {                                            // column t of L_s⁻¹ by forward substitution
        Li[t][t] = 1.0 / S[t][t];
        for (int i = t + 1; i < k; ++i) {
            double a = 0.0;
            for (int m = t; m < i; ++m) a = fma(S[i][m], Li[m][t], a);
            Li[i][t] = -a / S[i][i];
        }
    }
    __syncthreads();
    if (t < k) {
        double a = 0.0;
        for (int m = 0; m <= t; ++m) a = fma(Li[t][m], rv[m], a);
        uv[t] = a;
    }
    __syncthreads();
    for (int e = t; e < kp * kp; e += 256) {
        const int i = e / kp, j = e - i * kp;
        const bool in = i < k && j <= i;
        sm[e] = in ? S[i][j] : 0.0;
        sm[kp * kp + e] = in ? Li[i][j] : 0.0;
    }
    if (t < kp) {
        double b = 0.0;
        if (t < k)
            for (int i = t; i < k; ++i) b = fma(Li[i][t], uv[i], b);
        sm[2 * kp * kp + t] = b;
    }
    if (t == 0) {
        double ldet = 0.0, q = 0.0;
        for (int i = 0; i < k; ++i) {
            ldet += 2.0 * log(S[i][i]);
            q = fma(uv[i], uv[i], q);
        }
        scal[0] = ldet;
        scal[1] = q;
    }
}

// ---- the new rows ------------------------------------------------------------------------------------------------------------------
// Blocks 0 … ⌈N/64⌉ − 1: 64 old columns j each — L[N+i][j] = B[j][i], W[N+i][j] = WT[j][N+i] = −Σ_{m ≤ i} L_s⁻¹[i][m]·C[j][m],
// α'[j] = α[j] − Σ_m C[j][m]·β[m].  The last block: the k × k corner of the three matrices, α'[N + i] = β[i], zeros behind.
// Nothing when the pivot check failed.
constexpr int WR_COLS = 64;
__global__ void __launch_bounds__(256) ab_write_kernel(AppendBatchArgs p) {
    if (*p.info != 0) return;
    __shared__ double Li[APPEND_BATCH_MAX][AB_LDS], sC[WR_COLS][AB_LDS], beta[APPEND_BATCH_MAX];
    const int t = threadIdx.x;
    const int k = p.k, kp = p.kp;
    const int64_t N = p.N, ld = p.ld;
    const double* Ls = p.sm;
    const double* Lin = p.sm + kp * kp;
    const int nblk = (int)((N + WR_COLS - 1) / WR_COLS);
    if ((int)blockIdx.x == nblk) {
        for (int e = t; e < k * k; e += 256) {
            const int i = e / k, m = e - i * k;
            if (m > i) continue;
            const double w = Lin[i * kp + m];
            p.L[(N + i) * ld + N + m] = Ls[i * kp + m];
            p.W[(N + i) * ld + N + m] = w;
            p.WT[(N + m) * ld + N + i] = w;
        }
        for (int64_t j = N + t; j < p.cap; j += 256) p.alpha_new[j] = j < N + k ? p.sm[2 * kp * kp + (j - N)] : 0.0;
        return;
    }
    for (int e = t; e < k * k; e += 256) Li[e / k][e % k] = Lin[(e / k) * kp + e % k];
    if (t < k) beta[t] = p.sm[2 * kp * kp + t];
    const int64_t j0 = (int64_t)blockIdx.x * WR_COLS;
    for (int e = t; e < WR_COLS * kp; e += 256) {
        const int r = e / kp, c = e - r * kp;
        if (c < k) sC[r][c] = j0 + r < N ? p.C[(j0 + r) * kp + c] : 0.0;
    }
    __syncthreads();
    const int jl = t & 63, ig = t >> 6;                     // a lane per column, a wave per every fourth new row
    const int64_t j = j0 + jl;
    if (j >= N) return;
    for (int i = ig; i < k; i += 4) {
        double w = 0.0;
        for (int m = 0; m <= i; ++m) w = fma(Li[i][m], sC[jl][m], w);
        w = -w;
        p.L[(N + i) * ld + j] = p.B[j * kp + i];
        p.W[(N + i) * ld + j] = w;
        p.WT[j * ld + N + i] = w;
    }
    if (ig == 0) {
        double a = 0.0;
        for (int m = 0; m < k; ++m) a = fma(sC[jl][m], beta[m], a);
        p.alpha_new[j] = p.alpha_old[j] - a;
    }
}

}  // namespace

hipError_t launch_append_batch_points(const double* Xb, const double* yb, int k, int d, int dp, double s, double mean_c, double* Xraw_rows,
                                      double* Xs_rows, double* y_at, double* delta_at, int64_t* info, hipStream_t st) {
    if (k < 1 || k > APPEND_BATCH_MAX) return hipErrorInvalidValue;
    const int n = k * dp;
    hipLaunchKernelGGL(ab_points_kernel, dim3((n + 255) / 256), dim3(256), 0, st, Xb, yb, k, d, dp, s, mean_c, Xraw_rows, Xs_rows, y_at,
                       delta_at, info);
    return hipGetLastError();
}

hipError_t launch_append_batch_newcols(const double* Xs_new, const double* Xraw, double* Kb, int N, int k, int d, int dp, int family,
                                       double s, double sigma_f2, hipStream_t st) {
    if (k < 1 || k > APPEND_BATCH_MAX || N < 0) return hipErrorInvalidValue;
    const int kp = (int)pad_up(k, 16);
    const dim3 grid((unsigned)(((int64_t)(N + k) * kp + 255) / 256)), block(256);
    switch (family) {
        case ABO_KERNEL_SE: hipLaunchKernelGGL((ab_newcols_kernel<ABO_KERNEL_SE>), grid, block, 0, st, Xs_new, Xraw, Kb, N, k, kp, d, dp, s, sigma_f2); break;
        case ABO_KERNEL_MATERN52: hipLaunchKernelGGL((ab_newcols_kernel<ABO_KERNEL_MATERN52>), grid, block, 0, st, Xs_new, Xraw, Kb, N, k, kp, d, dp, s, sigma_f2); break;
        case ABO_KERNEL_MATERN72: hipLaunchKernelGGL((ab_newcols_kernel<ABO_KERNEL_MATERN72>), grid, block, 0, st, Xs_new, Xraw, Kb, N, k, kp, d, dp, s, sigma_f2); break;
        case ABO_KERNEL_MATERN32: hipLaunchKernelGGL((ab_newcols_kernel<ABO_KERNEL_MATERN32>), grid, block, 0, st, Xs_new, Xraw, Kb, N, k, kp, d, dp, s, sigma_f2); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

size_t tri_skinny_part_doubles(int N, int kp) { return (size_t)TS_SLICES * (size_t)N * (size_t)kp; }

hipError_t launch_tri_skinny(const double* Wm, int64_t ld, const double* V, double* out, double* part, int N, int kp, int lower,
                             hipStream_t s) {
    if (N <= 0) return hipSuccess;
    if (kp < 16 || kp > APPEND_BATCH_MAX || kp % 16 || ld % 4 || ld < pad_up(N, 16)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((N + TS_ROWS - 1) / TS_ROWS), TS_SLICES), block(256);
    switch (kp / 16) {
        case 1: hipLaunchKernelGGL((ts_product_kernel<1>), grid, block, 0, s, Wm, ld, V, part, N, lower); break;
        case 2: hipLaunchKernelGGL((ts_product_kernel<2>), grid, block, 0, s, Wm, ld, V, part, N, lower); break;
        case 3: hipLaunchKernelGGL((ts_product_kernel<3>), grid, block, 0, s, Wm, ld, V, part, N, lower); break;
        default: hipLaunchKernelGGL((ts_product_kernel<4>), grid, block, 0, s, Wm, ld, V, part, N, lower); break;
    }
    hipLaunchKernelGGL(ts_reduce_kernel, dim3((unsigned)(((int64_t)N * kp + 255) / 256)), block, 0, s, part, out, N, kp, lower);
    return hipGetLastError();
}

int append_batch_gram_blocks(int N) {
    const int g = (N + GRAM_CHUNK - 1) / GRAM_CHUNK;
    return g < 1 ? 1 : (g > 64 ? 64 : g);
}

hipError_t launch_append_batch_small(const double* Bm, const double* Kb, const double* alpha, const double* delta_b, int N, int k,
                                     double noise, double* gpart, double* sm, double* scal, int64_t* info, hipStream_t s) {
    if (k < 1 || k > APPEND_BATCH_MAX || N < 0) return hipErrorInvalidValue;
    const int kp = (int)pad_up(k, 16);
    const int G = append_batch_gram_blocks(N);
    const int rpb = (int)pad_up((N + G - 1) / G, GRAM_CHUNK);
    switch (kp / 16) {
        case 1: hipLaunchKernelGGL((ab_gram_kernel<1>), dim3(G), dim3(256), 0, s, Bm, Kb, alpha, N, rpb, gpart); break;
        case 2: hipLaunchKernelGGL((ab_gram_kernel<2>), dim3(G), dim3(256), 0, s, Bm, Kb, alpha, N, rpb, gpart); break;
        case 3: hipLaunchKernelGGL((ab_gram_kernel<3>), dim3(G), dim3(256), 0, s, Bm, Kb, alpha, N, rpb, gpart); break;
        default: hipLaunchKernelGGL((ab_gram_kernel<4>), dim3(G), dim3(256), 0, s, Bm, Kb, alpha, N, rpb, gpart); break;
    }
    hipLaunchKernelGGL(ab_small_kernel, dim3(1), dim3(256), 0, s, Kb + (int64_t)N * kp, gpart, G, delta_b, N, k, kp, noise, sm, scal, info);
    return hipGetLastError();
}

hipError_t launch_append_batch_write(const AppendBatchArgs& a, hipStream_t s) {
    if (a.k < 1 || a.k > APPEND_BATCH_MAX || a.kp != (int)pad_up(a.k, 16) || a.N + a.k > a.cap || a.cap > a.ld) return hipErrorInvalidValue;
    const unsigned nblk = (unsigned)((a.N + WR_COLS - 1) / WR_COLS);
    hipLaunchKernelGGL(ab_write_kernel, dim3(nblk + 1), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace abo
