// Thompson sampling: pathwise posterior sample paths (include/abo_hip.h: abo_paths_*).  No reference counterpart — the reference's
// acquisitions are EI, UCB, PI, GradientNormUCB and ensembles of them; this is an extension behind the same boundary, defined in the header.
//
// Matheron's rule (Wilson et al. 2020): with a prior draw f_s(x) = c + Σ_r w[s,r]·φ_r(x) in R random Fourier features and the EXACT
// kernel row k(z, X),
//     g_s(z) = f_s(z) + k(z, X)·v_s,     v_s = K̃⁻¹(y − f_s(X) − σ_n·ε_s)
// is a draw from the posterior.  For S paths over M candidates that is ONE product G = A·B,
//     row z of A = [k(z, x_1) … k(z, x_N), cos(ω_1·z/ℓ + b_1) … cos(ω_R·z/ℓ + b_R)]       generated, never stored
//     B = [V ; sqrt(2σ_f²/R)·wᵀ]                                                           (N4 + R4) × Sp, resident with the object
// on v_mfma_f64_16x16x4_f64.
//
// paths_eval_kernel<FAM, DP, NB>.  The instruction's operand map (A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], one f64 per lane;
// D[row = (l >> 4) + 4·reg][col = l & 15]) is the same for both operands, so the product is taken TRANSPOSED, Gᵀ = Bᵀ·Aᵀ: lane l owns
// candidate l & 15 of a 16-candidate tile and inner index l >> 4 of each 4-deep step, and the kernel value (or feature) it computes —
// abo_kappa.h's kappa_eval on kgen_core.h's squared-distance loop, candidate coordinates in registers — IS its fragment element: no LDS
// transpose.  The other operand, 16 paths × 4 rows of B, comes from an LDS slab of PT_KS rows that the workgroup's 4 waves and the
// PT_TPW tiles of each wave share (128 candidates per workgroup: B is re-read from L2 M/128 times).  The slab's row stride is padded
// 64 → 80 doubles and the training coordinates' DP → DP + 2: the two 32-lane groups of a ds_read_b64 then touch 64 distinct banks.
// Output rows are paths: for a fixed register 16 consecutive candidates of one path are 128 contiguous bytes.
// Accumulators: NB·PT_TPW blocks of 8 VGPRs (NB = 4, 64 paths: 64).  More than 64 paths run as groups of 64 columns (gridDim.y),
// each regenerating A.  One accumulation chain per output in a fixed order (training rows, then features), no atomics: two calls with
// the same inputs return the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <vector>

#include "../../include/abo_hip.h"
#include "abo_acq_dev.h"
#include "abo_internal.h"
#include "abo_kappa.h"
#include "abo_kernels.h"

struct abo_paths {
    abo_gp* gp = nullptr;                // retained
    int dev = 0, S = 0, R = 0, Sp = 0, NB = 0, d = 0, dp = 0, family = 0;
    int64_t N = 0, N4 = 0, R4 = 0;
    uint64_t gen = 0;                    // identity of the factor the paths were conditioned on
    double s = 0.0, sigma_f2 = 0.0, mean_c = 0.0;
    const double* Xs = nullptr;          // the model's scaled points (rows < N are immutable while the model is retained)
    void* buf = nullptr;                 // one block: Wf [R4][dp], phase [R4], B [(N4 + R4)][Sp]
    size_t cap = 0;
    double* Wf = nullptr; double* phase = nullptr; double* B = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    abo_paths_stats st{};
    // ---- abo_paths_append: the object follows the model through one-row appends
    double* Bt = nullptr; double* Bf = nullptr;   // training block [trows][Sp] (rows ≥ N zero) and feature block [R4][Sp]: B itself until the
    void* tbuf = nullptr; size_t tcap = 0;        // first append moves the training block into a buffer of its own with room to grow
    int64_t trows = 0;
    void* abuf = nullptr; size_t acap = 0;        // per-append scratch that stays: eps* [256], a_s [256], partial sums [AP_MAXBLK][Sp]
    hipEvent_t aev[3] = {nullptr, nullptr, nullptr};
    abo_paths_append_stats ast{};
    // ---- resident values on ONE candidate set (abo_paths_attach): G [S][Mp], the selection's partials and its result
    abo_cand* cset = nullptr;
    void* gbuf = nullptr; size_t gcap = 0;
    double* G = nullptr; double* ccol = nullptr; uint64_t* pkey = nullptr; int64_t* pidx = nullptr; double* tv1 = nullptr; int64_t* ti1 = nullptr;
    int64_t M = 0, Mp = 0, ntile = 0;
    uint64_t top_epoch = 0;                       // the set's mu_epoch the stored top-1 was selected under (0: none)
};

namespace abo {
namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));

constexpr int PT_MAXS = 256;
constexpr int PT_MAXR = 65536;
constexpr int PT_MAXD = 32;
constexpr int PT_KS = 64;                    // rows of B per LDS slab
constexpr int PT_LDB = 80;                   // slab row stride in doubles (64 columns + 16)
constexpr int PT_TPW = 2;                    // 16-candidate tiles per wave
constexpr int PT_CW = 4 * PT_TPW * 16;       // candidates per workgroup
constexpr size_t PT_CHUNK_BYTES = (size_t)128 << 20;   // of one S × chunk scratch array

struct PathsEvalArgs {
    const double* Xs;        // [≥ N4][DP] scaled training points
    const double* Z;         // [mc][d] raw candidates of this chunk
    const double* Wf;        // [R4][DP] ω, zero padded (the candidate is scaled by 1/ℓ instead)
    const double* phase;     // [R4]
    const double* Btrain;    // [N4][Sp] V (rows ≥ N zero)
    const double* Bfeat;     // [R4][Sp] sqrt(2σ_f²/R)·wᵀ (rows ≥ R zero)
    const double* excl;      // [mc] or nullptr: +Inf marks a candidate taken out (abo_cand_exclude) → g = +Inf
    double* out_g;           // [S][ldg] or nullptr
    double* out_neg;         // [S][ldn] or nullptr: −g, the score the selection orders by
    int64_t ldg, ldn, mc;
    int N, N4, R4, d, Sp, S;
    double s, sigma_f2, mean_c;
};

template <int FAM, int DP, int NB>
__global__ void __launch_bounds__(256) paths_eval_kernel(const PathsEvalArgs a) {
    constexpr int LDX = DP + 2;
    __shared__ double bs[PT_KS * PT_LDB];
    __shared__ double xs[PT_KS * LDX];
    __shared__ double ph[PT_KS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lk = lane >> 4;
    const int col0 = blockIdx.y * 16 * NB;
    const int64_t jb = (int64_t)blockIdx.x * PT_CW + wave * (PT_TPW * 16);
    double zc[PT_TPW][DP];
#pragma unroll
    for (int tt = 0; tt < PT_TPW; ++tt) {
        const int64_t j = jb + tt * 16 + li;
#pragma unroll
        for (int c = 0; c < DP; ++c) zc[tt][c] = (c < a.d && j < a.mc) ? a.Z[j * a.d + c] * a.s : 0.0;
    }
    d4_t acc[PT_TPW][NB];
#pragma unroll
    for (int tt = 0; tt < PT_TPW; ++tt)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[tt][nb] = d4_t{0.0, 0.0, 0.0, 0.0};

    // the training rows: A element = σ_f²·κ(‖x_k/ℓ − z/ℓ‖²)
    for (int k0 = 0; k0 < a.N4; k0 += PT_KS) {
        const int rows = min(PT_KS, a.N4 - k0);          // a multiple of 4
        __syncthreads();
        for (int e = t; e < rows * 16 * NB; e += 256) {
            const int r = e / (16 * NB), c = e % (16 * NB);
            bs[r * PT_LDB + c] = a.Btrain[(int64_t)(k0 + r) * a.Sp + col0 + c];
        }
        for (int e = t; e < rows * DP; e += 256) xs[(e / DP) * LDX + (e % DP)] = a.Xs[(int64_t)k0 * DP + e];
        __syncthreads();
        for (int kk = 0; kk < rows; kk += 4) {
            const int kr = kk + lk;
            double x[DP];
#pragma unroll
            for (int c = 0; c < DP; ++c) x[c] = xs[kr * LDX + c];
            const bool live = (k0 + kr) < a.N;           // rows N … N4 may hold the remains of a discarded append
#pragma unroll
            for (int tt = 0; tt < PT_TPW; ++tt) {
                double r2 = 0.0;
#pragma unroll
                for (int c = 0; c < DP; ++c) {
                    const double e = x[c] - zc[tt][c];
                    r2 = fma(e, e, r2);
                }
                const double kv = a.sigma_f2 * kappa_eval<FAM>(r2);
                const double av = live ? kv : 0.0;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[tt][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(bs[kr * PT_LDB + nb * 16 + li], av, acc[tt][nb], 0, 0, 0);
            }
        }
    }
    // the features: A element = cos(ω_r·z/ℓ + b_r)   (rows ≥ R of B are zero, and so are their ω and b)
    for (int k0 = 0; k0 < a.R4; k0 += PT_KS) {
        const int rows = min(PT_KS, a.R4 - k0);
        __syncthreads();
        for (int e = t; e < rows * 16 * NB; e += 256) {
            const int r = e / (16 * NB), c = e % (16 * NB);
            bs[r * PT_LDB + c] = a.Bfeat[(int64_t)(k0 + r) * a.Sp + col0 + c];
        }
        for (int e = t; e < rows * DP; e += 256) xs[(e / DP) * LDX + (e % DP)] = a.Wf[(int64_t)k0 * DP + e];
        if (t < rows) ph[t] = a.phase[k0 + t];
        __syncthreads();
        for (int kk = 0; kk < rows; kk += 4) {
            const int kr = kk + lk;
            double x[DP];
#pragma unroll
            for (int c = 0; c < DP; ++c) x[c] = xs[kr * LDX + c];
            const double b = ph[kr];
#pragma unroll
            for (int tt = 0; tt < PT_TPW; ++tt) {
                double arg = 0.0;
#pragma unroll
                for (int c = 0; c < DP; ++c) arg = fma(x[c], zc[tt][c], arg);
                const double av = cos(arg + b);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
                    acc[tt][nb] = __builtin_amdgcn_mfma_f64_16x16x4f64(bs[kr * PT_LDB + nb * 16 + li], av, acc[tt][nb], 0, 0, 0);
            }
        }
    }
    // D[row = lk + 4·reg][col = li]: path col0 + 16·nb + lk + 4·reg of candidate jb + 16·tt + li
#pragma unroll
    for (int tt = 0; tt < PT_TPW; ++tt) {
        const int64_t j = jb + tt * 16 + li;
        if (j >= a.mc) continue;
        const bool out = a.excl != nullptr && a.excl[j] == HUGE_VAL;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int path = col0 + nb * 16 + lk + 4 * r;
                if (path >= a.S) continue;
                const double g = out ? HUGE_VAL : a.mean_c + acc[tt][nb][r];
                if (a.out_g) a.out_g[(int64_t)path * a.ldg + j] = g;
                if (a.out_neg) a.out_neg[(int64_t)path * a.ldn + j] = -g;
            }
    }
}

template <int FAM, int DP>
hipError_t launch_eval_nb(const PathsEvalArgs& a, int NB, hipStream_t s) {
    const dim3 grid((unsigned)((a.mc + PT_CW - 1) / PT_CW), (unsigned)(a.Sp / (16 * NB))), block(256);
    switch (NB) {
        case 1: hipLaunchKernelGGL((paths_eval_kernel<FAM, DP, 1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((paths_eval_kernel<FAM, DP, 2>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((paths_eval_kernel<FAM, DP, 4>), grid, block, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int FAM>
hipError_t launch_eval_dp(const PathsEvalArgs& a, int dp, int NB, hipStream_t s) {
    switch (dp) {
        case 1: return launch_eval_nb<FAM, 1>(a, NB, s);
        case 2: return launch_eval_nb<FAM, 2>(a, NB, s);
        case 4: return launch_eval_nb<FAM, 4>(a, NB, s);
        case 8: return launch_eval_nb<FAM, 8>(a, NB, s);
        case 16: return launch_eval_nb<FAM, 16>(a, NB, s);
        case 32: return launch_eval_nb<FAM, 32>(a, NB, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_paths_eval(const PathsEvalArgs& a, int family, int dp, int NB, hipStream_t s) {
    if (a.mc < 1 || a.S < 1 || a.Sp % (16 * NB) != 0 || a.S > a.Sp || a.N4 % 4 != 0 || a.R4 % 4 != 0 || a.N > a.N4) return hipErrorInvalidValue;
    switch (family) {
        case ABO_KERNEL_SE: return launch_eval_dp<ABO_KERNEL_SE>(a, dp, NB, s);
        case ABO_KERNEL_MATERN52: return launch_eval_dp<ABO_KERNEL_MATERN52>(a, dp, NB, s);
        case ABO_KERNEL_MATERN72: return launch_eval_dp<ABO_KERNEL_MATERN72>(a, dp, NB, s);
        case ABO_KERNEL_MATERN32: return launch_eval_dp<ABO_KERNEL_MATERN32>(a, dp, NB, s);
        default: return hipErrorInvalidValue;
    }
}

// Wf[r][c] = ω[r][c], phase[r], B[N4 + r][s] = scale·w[s][r]   (padding stays zero: the block was cleared)
__global__ void paths_prep_kernel(const double* omega, const double* phase, const double* w, int R, int d, int dp, int S, int Sp,
                                  double scale, double* Wf, double* ph, double* Bfeat) {
    const int64_t n = (int64_t)R * (dp > Sp ? dp : Sp);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / (dp > Sp ? dp : Sp)), c = (int)(e % (dp > Sp ? dp : Sp));
        if (c < d) Wf[(int64_t)r * dp + c] = omega[(int64_t)r * d + c];
        if (c < S) Bfeat[(int64_t)r * Sp + c] = scale * w[(int64_t)c * R + r];
        if (c == 0) ph[r] = phase[r];
    }
}

// F[s][i] ← y[i] − F[s][i] − σ_n·ε[s][i]      (F holds f_s(x_i) on entry)
__global__ void paths_resid_kernel(double* F, int64_t ld, const double* y, const double* eps, int64_t N, int S, double sn) {
    const int64_t n = N * S;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = e / N, i = e % N;
        F[s * ld + i] = (y[i] - F[s * ld + i]) - sn * eps[s * N + i];
    }
}

// B[i][s] = V[s][i]
__global__ void paths_scatter_kernel(const double* V, int64_t ld, int64_t N, int S, int Sp, double* B) {
    const int64_t n = N * S;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / S, s = e % S;
        B[i * Sp + s] = V[s * ld + i];
    }
}

// the selection ordered −g: what it returns as values is g again; (NaN, −1) tails stay
__global__ void paths_negate_kernel(double* v, const int64_t* idx, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && idx[e] >= 0 && v[e] == v[e]) v[e] = -v[e];      // (a NaN stays the selection's canonical NaN, as in the tail)
}

// merged selection over the chunks' own: pos[s][i] indexes path s's list of nch·k (value, index) pairs
__global__ void paths_gather_kernel(const double* cv, const int64_t* ci, const int64_t* pos, int64_t per, int k, int S, double* tv, int64_t* ti) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)S * k) return;
    const int64_t s = e / k, p = pos[e];
    tv[e] = p < 0 ? __longlong_as_double(0x7ff8000000000000ll) : cv[s * per + p];
    ti[e] = p < 0 ? -1 : ci[s * per + p];
}

__global__ void paths_tail_kernel(double* tv, int64_t* ti, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) { tv[e] = __longlong_as_double(0x7ff8000000000000ll); ti[e] = -1; }
}

// ---- abo_paths_append -------------------------------------------------------------------------------------------------------------
// g_s(x*) of the paths as they stand, at the appended point x* (row N of the scaled points): Σ_i k(x*, x_i)·V[i][s] + Σ_r cos(ω_r·x*/ℓ + b_r)·Bf[r][s]
// as partial sums over slices of AP_ROWS rows (one workgroup each: its AP_ROWS operand values once into LDS, then 256 / cw row groups of cw
// columns, reduced in a fixed order), summed in slice order by paths_coef_kernel: no atomics, the same bits every time.
constexpr int AP_ROWS = 256;

struct PathsGxArgs {
    const double* Xs; const double* Wf; const double* phase; const double* Bt; const double* Bf;
    double* part;            // [nblk][Sp]
    int N, R4, d, dp, Sp, cw;
    double sigma_f2;
};

template <int FAM>
__global__ void __launch_bounds__(256) paths_gx_kernel(const PathsGxArgs a) {
    __shared__ double av[AP_ROWS];
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * AP_ROWS + t;
    const double* xstar = a.Xs + (int64_t)a.N * a.dp;
    double v = 0.0;
    if (i < a.N) {
        double r2 = 0.0;
        for (int c = 0; c < a.d; ++c) {
            const double e = a.Xs[i * a.dp + c] - xstar[c];
            r2 = fma(e, e, r2);
        }
        v = a.sigma_f2 * kappa_eval<FAM>(r2);
    } else if (i < (int64_t)a.N + a.R4) {
        const int64_t r = i - a.N;
        double arg = 0.0;
        for (int c = 0; c < a.d; ++c) arg = fma(a.Wf[r * a.dp + c], xstar[c], arg);
        v = cos(arg + a.phase[r]);                            // (rows ≥ R: ω = b = 0 and a zero row of Bf)
    }
    av[t] = v;
    __syncthreads();
    const int cw = a.cw, col = blockIdx.y * cw + t % cw, grp = t / cw, ngrp = 256 / cw;
    double acc = 0.0;
    for (int r = grp; r < AP_ROWS; r += ngrp) {
        const int64_t row = (int64_t)blockIdx.x * AP_ROWS + r;
        if (row >= (int64_t)a.N + a.R4) break;
        const double* b = row < a.N ? a.Bt + row * a.Sp : a.Bf + (row - a.N) * a.Sp;
        acc = fma(av[r], b[col], acc);
    }
    red[t] = acc;
    __syncthreads();
    if (grp == 0) {
        double sum = red[t];
        for (int g = 1; g < ngrp; ++g) sum += red[g * cw + t];
        a.part[(int64_t)blockIdx.x * a.Sp + col] = sum;
    }
}

// a_s = (y* − σ_n·ε*_s − g_s(x*)) / s²
__global__ void paths_coef_kernel(const double* part, int nblk, int Sp, int S, double mean_c, const double* ystar, const double* eps,
                                  double sn, double s2, double* coef) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double g = 0.0;
    for (int b = 0; b < nblk; ++b) g += part[(int64_t)b * Sp + s];
    g += mean_c;
    coef[s] = ((*ystar - sn * eps[s]) - g) / s2;
}

// V[i][s] += a_s·vext[i] (vext = [−u; 1]: V − a·u), row N ← a_s
__global__ void paths_vupd_kernel(double* Bt, const double* vext, const double* coef, int64_t N, int S, int Sp) {
    const int64_t n = (N + 1) * Sp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / Sp;
        const int s = (int)(e % Sp);
        if (s >= S) continue;
        Bt[e] = i < N ? fma(coef[s], vext[i], Bt[e]) : coef[s];
    }
}

// ---- resident values: G[s][j] += a_s·c(z_j) with the per-path arg-min fused --------------------------------------------------------
// The selection's order is abo_acq's rule on score = −g: NaN first, then the smallest g, ties → the lowest index.  g maps to a 64-bit
// key that orders the same way as an unsigned integer (NaN → 0; ±0 → one key), so a minimum over keys with the lowest index among
// equals IS the rule, whatever the shape of the reduction tree.
__device__ inline uint64_t sel_key(double g) {
    if (g != g) return 0ull;
    if (g == 0.0) g = 0.0;
    const uint64_t b = (uint64_t)__double_as_longlong(g);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

constexpr int RK_TILE = 1024;      // candidates per workgroup: 256 lanes × 4 doubles (two 16-byte loads per lane and path)
constexpr int RK_PPW = 4;          // paths per workgroup: 8 independent 16-byte loads per lane in flight

struct Rank1Args {
    double* G;               // [S][Mp], Mp a multiple of RK_TILE
    const double* c;         // [M] the down-date column (UPD only)
    const double* coef;      // [S] a_s (UPD only)
    const double* mu;        // [M] the set's stored μ: +Inf marks an excluded candidate → g counts as +Inf
    uint64_t* pkey; int64_t* pidx;    // [S][ntile] partial arg-min per path and tile
    int64_t M, Mp, ntile;
    int S;
};

// One workgroup: a tile of RK_TILE candidates × RK_PPW paths.  Streams c once per tile and G once (read + write); the partial arg-min of the
// UPDATED values goes to (pkey, pidx)[path][tile].  Lane l owns candidates 4l … 4l + 3 of the tile: indices ascend with the lane and with
// the wave, so "first lane / first wave holding the minimal key" is the lowest index.
template <bool UPD>
__global__ void __launch_bounds__(256) paths_rank1_argmin_kernel(const Rank1Args a) {
    typedef double d2_t __attribute__((ext_vector_type(2)));
    __shared__ uint64_t wk[4][RK_PPW];
    __shared__ int64_t wi[4][RK_PPW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t j0 = (int64_t)blockIdx.x * RK_TILE + 4 * t;
    const int s0 = blockIdx.y * RK_PPW;
    double cv[4];
    bool out[4], in[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        in[e] = j0 + e < a.M;
        cv[e] = (UPD && in[e]) ? a.c[j0 + e] : 0.0;
        out[e] = in[e] && a.mu[j0 + e] == HUGE_VAL;
    }
    d2_t g[RK_PPW][2];
#pragma unroll
    for (int p = 0; p < RK_PPW; ++p) {
        if (s0 + p >= a.S) continue;
        const d2_t* src = reinterpret_cast<const d2_t*>(a.G + (int64_t)(s0 + p) * a.Mp + j0);
        g[p][0] = src[0];
        g[p][1] = src[1];
    }
#pragma unroll
    for (int p = 0; p < RK_PPW; ++p) {
        if (s0 + p >= a.S) continue;                           // (uniform over the workgroup)
        if (UPD) {
            const double as = a.coef[s0 + p];
            g[p][0].x = fma(as, cv[0], g[p][0].x); g[p][0].y = fma(as, cv[1], g[p][0].y);
            g[p][1].x = fma(as, cv[2], g[p][1].x); g[p][1].y = fma(as, cv[3], g[p][1].y);
            d2_t* dst = reinterpret_cast<d2_t*>(a.G + (int64_t)(s0 + p) * a.Mp + j0);
            dst[0] = g[p][0];
            dst[1] = g[p][1];
        }
        const double ge[4] = {g[p][0].x, g[p][0].y, g[p][1].x, g[p][1].y};
        uint64_t key = ~0ull;
        int sub = 4;                                           // (no candidate of this lane is in the set)
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            const uint64_t k = sel_key(out[e] ? HUGE_VAL : ge[e]);
            if (in[e] && k <= key) { key = k; sub = e; }
        }
        uint64_t m = key;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint64_t other = __shfl_xor(m, o, 64);
            m = other < m ? other : m;
        }
        const uint64_t holders = __ballot(key == m && sub < 4);
        if (holders != 0ull && lane == __ffsll((unsigned long long)holders) - 1) { wk[wave][p] = key; wi[wave][p] = j0 + sub; }
        if (holders == 0ull && lane == 0) { wk[wave][p] = ~0ull; wi[wave][p] = -1; }
    }
    __syncthreads();
    if (t < RK_PPW && s0 + t < a.S) {
        uint64_t key = wk[0][t];
        int64_t idx = wi[0][t];
        for (int w = 1; w < 4; ++w)
            if (wi[w][t] >= 0 && (idx < 0 || wk[w][t] < key)) { key = wk[w][t]; idx = wi[w][t]; }
        a.pkey[(int64_t)(s0 + t) * a.ntile + blockIdx.x] = key;
        a.pidx[(int64_t)(s0 + t) * a.ntile + blockIdx.x] = idx;
    }
}

// per path: the partials under the strict total order (key, then index) — any tree gives the same winner; then the winner's value, the
// bits of G (an excluded candidate: +Inf; a NaN: the quiet NaN 0x7ff8…), index −1 and NaN for an empty set
__global__ void __launch_bounds__(256) paths_argmin_reduce_kernel(const Rank1Args a, double* tv, int64_t* ti) {
    __shared__ uint64_t rk[256];
    __shared__ int64_t ri[256];
    const int t = threadIdx.x, s = blockIdx.x;
    uint64_t key = ~0ull;
    int64_t idx = -1;
    for (int64_t b = t; b < a.ntile; b += 256) {
        const uint64_t k = a.pkey[(int64_t)s * a.ntile + b];
        const int64_t i = a.pidx[(int64_t)s * a.ntile + b];
        if (i >= 0 && (idx < 0 || k < key || (k == key && i < idx))) { key = k; idx = i; }
    }
    rk[t] = key; ri[t] = idx;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) {
            const uint64_t k = rk[t + o];
            const int64_t i = ri[t + o];
            if (i >= 0 && (ri[t] < 0 || k < rk[t] || (k == rk[t] && i < ri[t]))) { rk[t] = k; ri[t] = i; }
        }
        __syncthreads();
    }
    if (t == 0) {
        const int64_t i = ri[0];
        double v = __longlong_as_double(0x7ff8000000000000ll);
        if (i >= 0) {
            const double g = a.mu[i] == HUGE_VAL ? HUGE_VAL : a.G[(int64_t)s * a.Mp + i];
            if (g == g) v = g;
        }
        tv[s] = v; ti[s] = i;
    }
}

// out[s][j] = G[s][j], +Inf where the set's stored μ is +Inf (sign = −1: the negated score the k > 1 selection orders by)
__global__ void paths_resident_copy_kernel(const double* G, int64_t Mp, const double* mu, int64_t M, int S, double sign, double* out, int64_t ld) {
    const int64_t n = (int64_t)S * M;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = e / M, j = e % M;
        const double g = mu[j] == HUGE_VAL ? HUGE_VAL : G[s * Mp + j];
        out[s * ld + j] = sign * g;
    }
}

__global__ void paths_top1_emit_kernel(const double* tv, const int64_t* ti, int S, int64_t idx_base, double* ov, int64_t* oi) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) { ov[s] = tv[s]; oi[s] = ti[s] < 0 ? -1 : ti[s] + idx_base; }
}

inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 65535); }

int32_t fail(int32_t code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return set_error(code, buf);
}

#define PCHK(expr)                                                                                                         \
    do {                                                                                                                   \
        const hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess)                                                                                              \
            return fail(e_ == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                                               \
    } while (0)

size_t take(size_t& off, size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
}

// scratch of one call: the stream is drained before the block goes back to the pool, on every exit path
struct Scratch {
    int dev; hipStream_t s; void* p = nullptr; size_t cap = 0;
    Scratch(int dv, hipStream_t st) : dev(dv), s(st) {}
    ~Scratch() { if (p) { (void)stream_wait(s); scratch_free(dev, p, cap); } }
    hipError_t get(size_t bytes) { return scratch_alloc(dev, bytes ? bytes : 256, &p, &cap); }
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(p) + off); }
};

PathsEvalArgs eval_args(const abo_paths* p) {
    PathsEvalArgs a{};
    a.Xs = p->Xs; a.Wf = p->Wf; a.phase = p->phase; a.Btrain = p->Bt; a.Bfeat = p->Bf;
    a.N = (int)p->N; a.N4 = (int)p->N4; a.R4 = (int)p->R4; a.d = p->d; a.Sp = p->Sp; a.S = p->S;
    a.s = p->s; a.sigma_f2 = p->sigma_f2; a.mean_c = p->mean_c;
    return a;
}

// g_s over M candidates on the device (Zd), chunk by chunk; excl: the resident set's stored μ (or nullptr)
int32_t paths_run(abo_paths* p, const double* Zd, int64_t M, const double* excl, int64_t idx_base, double* values, int32_t k,
                  double* top_val, int64_t* top_idx, int32_t out_space) {
    hipStream_t s = gp_stream(p->gp);
    const int S = p->S, d = p->d;
    const bool host = out_space == ABO_HOST;
    if (M == 0) {
        if (k > 0) {
            Scratch sc(p->dev, s);
            size_t off = 0;
            const size_t o_tv = take(off, sizeof(double) * S * k), o_ti = take(off, sizeof(int64_t) * S * k);
            if (host) PCHK(sc.get(off));
            double* tv = host ? sc.at<double>(o_tv) : top_val;
            int64_t* ti = host ? sc.at<int64_t>(o_ti) : top_idx;
            hipLaunchKernelGGL(paths_tail_kernel, dim3((unsigned)(((int64_t)S * k + 255) / 256)), dim3(256), 0, s, tv, ti, (int64_t)S * k);
            PCHK(hipGetLastError());
            if (host) {
                PCHK(hipMemcpyAsync(top_val, tv, sizeof(double) * S * k, hipMemcpyDeviceToHost, s));
                PCHK(hipMemcpyAsync(top_idx, ti, sizeof(int64_t) * S * k, hipMemcpyDeviceToHost, s));
            }
            PCHK(stream_wait(s));
        }
        return ABO_OK;
    }
    // chunks of Mc candidates: one S × chunk scratch array stays within PT_CHUNK_BYTES.  The remainder is a chunk of its own when it holds
    // at least k candidates, else the last chunk takes it (at most k − 1 more): no chunk's own selection has a (NaN, −1) tail
    // unless the call has one chunk
    int64_t Mc = (int64_t)(PT_CHUNK_BYTES / (sizeof(double) * S)) / PT_CW * PT_CW;
    if (Mc < k) Mc = pad_up(k, PT_CW);
    int64_t nch = (M + Mc - 1) / Mc;
    if (nch > 1 && M - (nch - 1) * Mc < k) --nch;
    const int64_t mcmax = nch == 1 ? M : std::max(Mc, M - (nch - 1) * Mc), ldc = pad_up(mcmax, 2);
    const bool g_scratch = values && host, n_scratch = k > 0;
    const int64_t per = nch * k;
    const int64_t we = k > 0 ? topk_workspace_entries(std::max(mcmax, per), k) : 0;
    size_t off = 0;
    const size_t o_g = take(off, g_scratch ? sizeof(double) * S * ldc : 0), o_n = take(off, n_scratch ? sizeof(double) * S * ldc : 0),
                 o_k0 = take(off, sizeof(uint64_t) * we), o_k1 = take(off, sizeof(uint64_t) * we), o_i0 = take(off, sizeof(int64_t) * we),
                 o_i1 = take(off, sizeof(int64_t) * we), o_cv = take(off, nch > 1 ? sizeof(double) * S * per : 0),
                 o_ci = take(off, nch > 1 ? sizeof(int64_t) * S * per : 0), o_pv = take(off, nch > 1 ? sizeof(double) * S * k : 0),
                 o_pi = take(off, nch > 1 ? sizeof(int64_t) * S * k : 0), o_tv = take(off, host ? sizeof(double) * S * k : 0),
                 o_ti = take(off, host ? sizeof(int64_t) * S * k : 0);
    Scratch sc(p->dev, s);
    PCHK(sc.get(off));
    TopkWork w{{sc.at<uint64_t>(o_k0), sc.at<uint64_t>(o_k1)}, {sc.at<int64_t>(o_i0), sc.at<int64_t>(o_i1)}};
    double* tv = host ? sc.at<double>(o_tv) : top_val;
    int64_t* ti = host ? sc.at<int64_t>(o_ti) : top_idx;
    PathsEvalArgs a = eval_args(p);
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t j0 = c * Mc, mc = c == nch - 1 ? M - j0 : Mc;
        a.Z = Zd + j0 * d; a.excl = excl ? excl + j0 : nullptr; a.mc = mc;
        a.out_g = nullptr; a.out_neg = nullptr;
        if (values) {
            if (host) { a.out_g = sc.at<double>(o_g); a.ldg = ldc; }
            else { a.out_g = values + j0; a.ldg = M; }
        }
        if (k > 0) { a.out_neg = sc.at<double>(o_n); a.ldn = ldc; }
        if (a.out_g || a.out_neg) PCHK(launch_paths_eval(a, p->family, p->dp, p->NB, s));
        if (values && host)
            PCHK(hipMemcpy2DAsync(values + j0, sizeof(double) * M, a.out_g, sizeof(double) * ldc, sizeof(double) * mc, S, hipMemcpyDeviceToHost, s));
        for (int ps = 0; ps < S && k > 0; ++ps) {
            double* cv = nch > 1 ? sc.at<double>(o_cv) + ps * per + c * k : tv + (int64_t)ps * k;
            int64_t* ci = nch > 1 ? sc.at<int64_t>(o_ci) + ps * per + c * k : ti + (int64_t)ps * k;
            PCHK(launch_topk(a.out_neg + ps * ldc, mc, k, idx_base + j0, w, cv, ci, s));
        }
    }
    if (k > 0) {
        const int64_t n = (int64_t)S * k;
        if (nch > 1) {
            // within a path's list equal scores stand in ascending index order (each chunk's selection is, and the chunks follow each
            // other), so the stable selection over the list is the selection over all candidates
            for (int ps = 0; ps < S; ++ps)
                PCHK(launch_topk(sc.at<double>(o_cv) + ps * per, per, k, 0, w, sc.at<double>(o_pv) + (int64_t)ps * k,
                                 sc.at<int64_t>(o_pi) + (int64_t)ps * k, s));
            hipLaunchKernelGGL(paths_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sc.at<double>(o_cv), sc.at<int64_t>(o_ci),
                               sc.at<int64_t>(o_pi), per, k, S, tv, ti);
            PCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(paths_negate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tv, ti, n);
        PCHK(hipGetLastError());
        if (host) {
            PCHK(hipMemcpyAsync(top_val, tv, sizeof(double) * n, hipMemcpyDeviceToHost, s));
            PCHK(hipMemcpyAsync(top_idx, ti, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
        }
    }
    return ABO_OK;
}

int32_t check_eval_args(const char* fn, const abo_paths* p, int32_t k, const double* top_val, const int64_t* top_idx,
                        int32_t out_space) {
    if (!p) return fail(ABO_EINVAL, "%s: null paths object", fn);
    if (k < 0) return fail(ABO_EINVAL, "%s: k = %d is negative", fn, k);
    if (k > 0 && (!top_val || !top_idx)) return fail(ABO_EINVAL, "%s: k > 0 needs top_val and top_idx", fn);
    if (out_space != ABO_HOST && out_space != ABO_DEVICE) return fail(ABO_EINVAL, "%s: unknown memory space %d", fn, out_space);
    return ABO_OK;
}

// the model must still be the one the paths were conditioned on (abo_fit on the retained handle replaces its factor)
int32_t check_model(const char* fn, abo_paths* p) {
    FactorView fv{};
    GpState gs{};
    if (!gp_state(p->gp, &gs) || !gp_factor_view(p->gp, &fv) || fv.gen != p->gen || gs.rows != p->N)
        return fail(ABO_EINVAL, "%s: the model handle was conditioned on other data (abo_fit) after abo_paths_create", fn);
    return ABO_OK;
}

int32_t timed_eval(abo_paths* p, const double* Zd, int64_t M, const double* excl, int64_t idx_base, double* values, int32_t k,
                   double* top_val, int64_t* top_idx, int32_t out_space) {
    hipStream_t s = gp_stream(p->gp);
    PCHK(hipEventRecord(p->ev[2], s));
    const int32_t rc = paths_run(p, Zd, M, excl, idx_base, values, k, top_val, top_idx, out_space);
    if (rc) return rc;
    PCHK(hipEventRecord(p->ev[3], s));
    PCHK(stream_wait(s));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p->ev[2], p->ev[3]) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    p->st.eval_ms = ms;
    p->st.eval_flop = 2.0 * (double)(p->N + p->R) * (double)M * (double)p->S;
    return ABO_OK;
}

void paths_free(abo_paths* p) {
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->aev) if (e) (void)hipEventDestroy(e);
    if (p->buf) scratch_free(p->dev, p->buf, p->cap);
    if (p->tbuf) scratch_free(p->dev, p->tbuf, p->tcap);
    if (p->abuf) scratch_free(p->dev, p->abuf, p->acap);
    if (p->gbuf) scratch_free(p->dev, p->gbuf, p->gcap);
    if (p->gp) abo_destroy(p->gp);
    delete p;
}

template <int FAM>
void launch_gx_fam(const PathsGxArgs& a, int nblk, hipStream_t s) {
    hipLaunchKernelGGL((paths_gx_kernel<FAM>), dim3((unsigned)nblk, (unsigned)(a.Sp / a.cw)), dim3(256), 0, s, a);
}

hipError_t launch_paths_gx(const PathsGxArgs& a, int family, int nblk, hipStream_t s) {
    switch (family) {
        case ABO_KERNEL_SE: launch_gx_fam<ABO_KERNEL_SE>(a, nblk, s); break;
        case ABO_KERNEL_MATERN52: launch_gx_fam<ABO_KERNEL_MATERN52>(a, nblk, s); break;
        case ABO_KERNEL_MATERN72: launch_gx_fam<ABO_KERNEL_MATERN72>(a, nblk, s); break;
        case ABO_KERNEL_MATERN32: launch_gx_fam<ABO_KERNEL_MATERN32>(a, nblk, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

void drop_resident(abo_paths* p) {
    if (p->gbuf) scratch_free(p->dev, p->gbuf, p->gcap);
    p->gbuf = nullptr; p->gcap = 0; p->G = nullptr; p->ccol = nullptr; p->pkey = nullptr; p->pidx = nullptr; p->tv1 = nullptr; p->ti1 = nullptr;
    p->cset = nullptr; p->M = p->Mp = p->ntile = 0; p->top_epoch = 0;
}

Rank1Args rank1_args(const abo_paths* p) {
    Rank1Args a{};
    a.G = p->G; a.mu = cand_mu(p->cset); a.pkey = p->pkey; a.pidx = p->pidx; a.M = p->M; a.Mp = p->Mp; a.ntile = p->ntile; a.S = p->S;
    return a;
}

// the selection over the resident values (UPD: behind the rank-1 update, in the same launch), then the per-path reduction of its partials
int32_t resident_select(abo_paths* p, const double* col, const double* coef, hipStream_t s) {
    Rank1Args a = rank1_args(p);
    a.c = col; a.coef = coef;
    if (p->M > 0) {
        const dim3 grid((unsigned)p->ntile, (unsigned)((p->S + RK_PPW - 1) / RK_PPW));
        if (col) hipLaunchKernelGGL((paths_rank1_argmin_kernel<true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((paths_rank1_argmin_kernel<false>), grid, dim3(256), 0, s, a);
        PCHK(hipGetLastError());
    } else {
        PCHK(hipMemsetAsync(p->pidx, 0xff, sizeof(int64_t) * p->S * p->ntile, s));      // an empty set: no tile has a candidate (index −1)
    }
    hipLaunchKernelGGL(paths_argmin_reduce_kernel, dim3((unsigned)p->S), dim3(256), 0, s, a, p->tv1, p->ti1);
    PCHK(hipGetLastError());
    CandSync cs{};
    cand_sync(p->cset, &cs);
    p->top_epoch = cs.mu_epoch;
    return ABO_OK;
}

}  // namespace
}  // namespace abo

using namespace abo;

extern "C" {

int32_t abo_paths_create(abo_gp* gp, int32_t S, int32_t R, const double* omega, const double* phase, const double* w, const double* eps,
                         int32_t space, void** out) {
    // every argument check comes before the handle is looked at
    if (!gp || !omega || !phase || !w || !eps || !out) return fail(ABO_EINVAL, "abo_paths_create: null argument");
    if (S < 1 || S > PT_MAXS) return fail(ABO_EINVAL, "abo_paths_create: S = %d sample paths outside 1..%d", S, PT_MAXS);
    if (R < 1 || R > PT_MAXR) return fail(ABO_EINVAL, "abo_paths_create: R = %d random features outside 1..%d", R, PT_MAXR);
    if (space != ABO_HOST && space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_paths_create: unknown memory space %d", space);
    GpState gs{};
    FactorView fv{};
    if (!gp_state(gp, &gs) || !gp_factor_view(gp, &fv))
        return fail(ABO_EINVAL, "abo_paths_create: surrogate is not conditioned on data yet (call abo_fit first)");
    if (gs.p_out > 1)
        return fail(ABO_EINVAL, "abo_paths_create: sample paths exist for the standard GP only, not for a gradient-enhanced model");
    if (gs.d > PT_MAXD) return fail(ABO_EINVAL, "abo_paths_create: d = %d inputs; sample paths are generated for d <= %d", gs.d, PT_MAXD);
    const abo_params& prm = gp_params(gp);
    const int dev = gs.device, d = gs.d;
    const int64_t N = gs.rows;
    PCHK(hipSetDevice(dev));
    abo_paths* p = new (std::nothrow) abo_paths();
    if (!p) return fail(ABO_ENOMEM, "abo_paths_create: host allocation failed");
    struct Guard { abo_paths* p; ~Guard() { if (p) paths_free(p); } } guard{p};
    p->dev = dev; p->S = S; p->R = R; p->d = d; p->dp = fv.dp; p->family = prm.family; p->N = N; p->gen = fv.gen; p->Xs = fv.Xs;
    p->Sp = S <= 16 ? 16 : S <= 32 ? 32 : (int)pad_up(S, 64);
    p->NB = p->Sp >= 64 ? 4 : p->Sp / 16;
    p->N4 = pad_up(N, 4); p->R4 = pad_up(R, 4);
    p->s = 1.0 / prm.ell; p->sigma_f2 = prm.sigma_f2; p->mean_c = prm.mean_c;
    for (hipEvent_t& e : p->ev) PCHK(hipEventCreate(&e));
    size_t off = 0;
    const size_t o_wf = take(off, sizeof(double) * p->R4 * p->dp), o_ph = take(off, sizeof(double) * p->R4),
                 o_b = take(off, sizeof(double) * (p->N4 + p->R4) * p->Sp);
    PCHK(scratch_alloc(dev, off, &p->buf, &p->cap));
    abo_retain(gp);
    p->gp = gp;
    char* base = static_cast<char*>(p->buf);
    p->Wf = reinterpret_cast<double*>(base + o_wf); p->phase = reinterpret_cast<double*>(base + o_ph); p->B = reinterpret_cast<double*>(base + o_b);
    p->Bt = p->B; p->Bf = p->B + p->N4 * p->Sp; p->trows = p->N4;
    hipStream_t s = gp_stream(gp);
    PCHK(hipEventRecord(p->ev[0], s));
    PCHK(hipMemsetAsync(p->buf, 0, off, s));
    // scratch: the caller's host arrays, and two N-vectors per path (leading dimension ldv: launch_trmv reads its vector in pairs)
    const int64_t ldv = pad_up(N, TB);
    const bool host = space == ABO_HOST;
    size_t so = 0;
    const size_t o_om = take(so, host ? sizeof(double) * R * d : 0), o_p = take(so, host ? sizeof(double) * R : 0),
                 o_w = take(so, host ? sizeof(double) * S * R : 0), o_e = take(so, host ? sizeof(double) * S * N : 0),
                 o_f = take(so, sizeof(double) * S * ldv), o_t = take(so, sizeof(double) * S * ldv);
    Scratch sc(dev, s);
    PCHK(sc.get(so));
    if (host) {
        PCHK(hipMemcpyAsync(sc.at<double>(o_om), omega, sizeof(double) * R * d, hipMemcpyHostToDevice, s));
        PCHK(hipMemcpyAsync(sc.at<double>(o_p), phase, sizeof(double) * R, hipMemcpyHostToDevice, s));
        PCHK(hipMemcpyAsync(sc.at<double>(o_w), w, sizeof(double) * S * R, hipMemcpyHostToDevice, s));
        PCHK(hipMemcpyAsync(sc.at<double>(o_e), eps, sizeof(double) * S * N, hipMemcpyHostToDevice, s));
        omega = sc.at<double>(o_om); phase = sc.at<double>(o_p); w = sc.at<double>(o_w); eps = sc.at<double>(o_e);
    }
    double* F = sc.at<double>(o_f);
    double* T = sc.at<double>(o_t);
    PCHK(hipMemsetAsync(F, 0, (o_t - o_f) + sizeof(double) * S * ldv, s));
    const int wide = p->dp > p->Sp ? p->dp : p->Sp;
    hipLaunchKernelGGL(paths_prep_kernel, dim3(grid_for((int64_t)R * wide)), dim3(256), 0, s, omega, phase, w, R, d, p->dp, S, p->Sp,
                       std::sqrt(2.0 * prm.sigma_f2 / (double)R), p->Wf, p->phase, p->B + p->N4 * p->Sp);
    PCHK(hipGetLastError());
    // f_s(X): the evaluation pass on Z = X with the feature half only
    PathsEvalArgs a = eval_args(p);
    a.N = 0; a.N4 = 0; a.Z = gs.Xraw; a.mc = N; a.out_g = F; a.ldg = ldv;
    PCHK(launch_paths_eval(a, p->family, p->dp, p->NB, s));
    hipLaunchKernelGGL(paths_resid_kernel, dim3(grid_for(N * S)), dim3(256), 0, s, F, ldv, gs.ybuf, eps, N, S, std::sqrt(prm.noise_var));
    PCHK(hipGetLastError());
    // v_s = L⁻ᵀ(L⁻¹ r_s): the bordered append's two triangular mat-vecs, once per path (rows and columns < N only)
    for (int ps = 0; ps < S; ++ps) {
        PCHK(launch_trmv(fv.W, fv.ld, F + ps * ldv, T + ps * ldv, (int)N, 1, s));
        PCHK(launch_trmv(fv.WT, fv.ld, T + ps * ldv, F + ps * ldv, (int)N, 0, s));
    }
    hipLaunchKernelGGL(paths_scatter_kernel, dim3(grid_for(N * S)), dim3(256), 0, s, F, ldv, N, S, p->Sp, p->B);
    PCHK(hipGetLastError());
    PCHK(hipEventRecord(p->ev[1], s));
    PCHK(stream_wait(s));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p->ev[0], p->ev[1]) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
    p->st.create_ms = ms; p->st.S = S; p->st.R = R; p->st.N = N;
    guard.p = nullptr;
    *out = p;
    return ABO_OK;
}

int32_t abo_paths_destroy(void* paths) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p || exiting()) return ABO_OK;
    hipError_t e = hipSetDevice(p->dev);
    if (e == hipSuccess) e = stream_wait(gp_stream(p->gp));
    if (gone(e)) return ABO_OK;
    (void)hipGetLastError();
    paths_free(p);
    return ABO_OK;
}

int32_t abo_paths_eval(void* paths, const double* Z, int64_t M, int32_t d, int32_t z_space, int64_t idx_base, double* values, int32_t k,
                       double* top_val, int64_t* top_idx, int32_t out_space) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    int32_t rc = check_eval_args("abo_paths_eval", p, k, top_val, top_idx, out_space);
    if (rc) return rc;
    if (M < 0 || (M > 0 && !Z)) return fail(ABO_EINVAL, "abo_paths_eval: bad candidate buffer");
    if (z_space != ABO_HOST && z_space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_paths_eval: unknown memory space %d", z_space);
    if (d != p->d) return fail(ABO_EDIM, "DimensionMismatch: candidate dimension %d, model dimension %d", d, p->d);
    rc = check_model("abo_paths_eval", p);
    if (rc) return rc;
    PCHK(hipSetDevice(p->dev));
    hipStream_t s = gp_stream(p->gp);
    Scratch zs(p->dev, s);
    const double* Zd = Z;
    if (z_space == ABO_HOST && M > 0) {
        PCHK(zs.get(sizeof(double) * M * d));
        PCHK(hipMemcpyAsync(zs.p, Z, sizeof(double) * M * d, hipMemcpyHostToDevice, s));
        Zd = zs.at<double>(0);
    }
    return timed_eval(p, Zd, M, nullptr, idx_base, values, k, top_val, top_idx, out_space);
}

int32_t abo_paths_eval_cand(void* paths, abo_cand* c, int64_t idx_base, double* values, int32_t k, double* top_val, int64_t* top_idx,
                            int32_t out_space) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    int32_t rc = check_eval_args("abo_paths_eval_cand", p, k, top_val, top_idx, out_space);
    if (rc) return rc;
    if (!c) return fail(ABO_EINVAL, "abo_paths_eval_cand: null candidate set");
    if (cand_dim(c) != p->d) return fail(ABO_EDIM, "DimensionMismatch: candidate dimension %d, model dimension %d", cand_dim(c), p->d);
    if (cand_device(c) != p->dev) return fail(ABO_EINVAL, "abo_paths_eval_cand: the candidate set lives on device %d, the model on %d", cand_device(c), p->dev);
    rc = check_model("abo_paths_eval_cand", p);
    if (rc) return rc;
    PCHK(hipSetDevice(p->dev));
    return timed_eval(p, cand_points(c), cand_size(c), cand_mu(c), idx_base, values, k, top_val, top_idx, out_space);
}

int32_t abo_paths_append(void* paths, abo_gp* gp2, const double* eps_new, int32_t space) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    // every argument check comes before the handles are looked at, every refusal before any device work
    if (!p || !gp2 || !eps_new) return fail(ABO_EINVAL, "abo_paths_append: null argument");
    if (space != ABO_HOST && space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_paths_append: unknown memory space %d", space);
    const int S = p->S;
    if (space == ABO_HOST)
        for (int i = 0; i < S; ++i)
            if (!std::isfinite(eps_new[i])) return fail(ABO_EINVAL, "abo_paths_append: eps_new[%d] is not finite", i);
    int32_t rc = check_model("abo_paths_append", p);
    if (rc) return rc;
    GpState gs{};
    FactorView fv{};
    AppendView av{};
    if (!gp_state(gp2, &gs) || !gp_factor_view(gp2, &fv))
        return fail(ABO_EINVAL, "abo_paths_append: the new model is not conditioned on data");
    if (gs.p_out > 1) return fail(ABO_EINVAL, "abo_paths_append: sample paths exist for the standard GP only, not for a gradient-enhanced model");
    if (gs.d != p->d) return fail(ABO_EINVAL, "abo_paths_append: the new model has %d inputs, the paths' model %d", gs.d, p->d);
    if (fv.gen != p->gen)
        return fail(ABO_EINVAL, "abo_paths_append: the new model does not share the factor of the paths' model (another lineage, or the "
                                "append fell back to a refit): make new paths with abo_paths_create");
    if (gs.rows != p->N + 1)
        return fail(ABO_EINVAL, "abo_paths_append: the new model has %lld points, the paths' model %lld: it must be exactly ONE append ahead "
                                "(k appends are k calls, in append order)", (long long)gs.rows, (long long)p->N);
    if (!gp_append_view(gp2, &av))
        return fail(ABO_EINVAL, "abo_paths_append: the new model was not made by abo_append (a refit leaves no bordered-append state)");
    if (!(av.s2 > 0.0)) return fail(ABO_EINVAL, "abo_paths_append: the append's pivot %g is not positive", av.s2);
    const abo_params& prm = gp_params(gp2);
    if (1.0 / prm.ell != p->s || prm.sigma_f2 != p->sigma_f2 || prm.mean_c != p->mean_c || prm.family != p->family)
        return fail(ABO_EINVAL, "abo_paths_append: the new model's hyper-parameters differ from the paths' model");
    abo_cand* c = p->cset;
    if (c) {
        CandSync cs{};
        cand_sync(c, &cs);
        if (cs.gen != fv.gen || cs.N != gs.rows)
            return fail(ABO_EINVAL, "abo_paths_append: the attached candidate set is not in sync with the new model (abo_cand_downdate(gp2, c) "
                                    "comes first)");
    }
    PCHK(hipSetDevice(p->dev));
    hipStream_t s = gp_stream(gp2);
    const int64_t N = p->N, N4n = pad_up(N + 1, 4);
    const int Sp = p->Sp;
    for (hipEvent_t& e : p->aev) if (!e) PCHK(hipEventCreate(&e));
    // row capacity of the training block: a buffer of its own from the first append on, doubled when it is full (rows ≥ N stay zero)
    if (N4n > p->trows || !p->tbuf) {
        const int64_t rows = pad_up(std::max<int64_t>(2 * N4n, N4n + 256), 4);
        void* nb = nullptr;
        size_t ncap = 0;
        PCHK(scratch_alloc(p->dev, sizeof(double) * rows * Sp, &nb, &ncap));
        hipError_t e = hipMemsetAsync(nb, 0, sizeof(double) * rows * Sp, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nb, p->Bt, sizeof(double) * p->N4 * Sp, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = stream_wait(s);
        if (e != hipSuccess) { scratch_free(p->dev, nb, ncap); PCHK(e); }
        if (p->tbuf) scratch_free(p->dev, p->tbuf, p->tcap);
        p->tbuf = nb; p->tcap = ncap; p->trows = rows; p->Bt = static_cast<double*>(nb);
    }
    const int nblk = (int)((N + p->R4 + AP_ROWS - 1) / AP_ROWS);
    size_t off = 0;
    const size_t o_eps = take(off, sizeof(double) * 256), o_coef = take(off, sizeof(double) * 256), o_part = take(off, sizeof(double) * nblk * Sp);
    if (off > p->acap) {
        if (p->abuf) scratch_free(p->dev, p->abuf, p->acap);
        p->abuf = nullptr; p->acap = 0;
        PCHK(scratch_alloc(p->dev, 2 * off, &p->abuf, &p->acap));
    }
    char* ab = static_cast<char*>(p->abuf);
    double* eps_d = reinterpret_cast<double*>(ab + o_eps);
    double* coef = reinterpret_cast<double*>(ab + o_coef);
    double* part = reinterpret_cast<double*>(ab + o_part);
    PCHK(hipMemcpyAsync(eps_d, eps_new, sizeof(double) * S, space == ABO_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    PCHK(hipEventRecord(p->aev[0], s));
    PathsGxArgs ga{};
    ga.Xs = fv.Xs; ga.Wf = p->Wf; ga.phase = p->phase; ga.Bt = p->Bt; ga.Bf = p->Bf; ga.part = part;
    ga.N = (int)N; ga.R4 = (int)p->R4; ga.d = p->d; ga.dp = p->dp; ga.Sp = Sp; ga.cw = Sp < 64 ? Sp : 64; ga.sigma_f2 = p->sigma_f2;
    PCHK(launch_paths_gx(ga, p->family, nblk, s));
    hipLaunchKernelGGL(paths_coef_kernel, dim3(1), dim3(256), 0, s, part, nblk, Sp, S, p->mean_c, gs.ybuf + N, eps_d,
                       std::sqrt(prm.noise_var), av.s2, coef);
    PCHK(hipGetLastError());
    hipLaunchKernelGGL(paths_vupd_kernel, dim3(grid_for((N + 1) * Sp)), dim3(256), 0, s, p->Bt, av.vext, coef, N, S, Sp);
    PCHK(hipGetLastError());
    PCHK(hipEventRecord(p->aev[1], s));
    int route = -1;
    if (c) {
        const double* col = nullptr;
        if (p->M > 0) {
            rc = cand_downdate_column(gp2, c, p->ccol, &col, &route);
            if (rc) { (void)stream_wait(s); return rc; }
        }
        rc = resident_select(p, p->M > 0 ? col : nullptr, coef, s);
        if (rc) { (void)stream_wait(s); return rc; }
    }
    PCHK(hipEventRecord(p->aev[2], s));
    PCHK(stream_wait(s));
    float m0 = 0.f, m1 = 0.f;
    if (hipEventElapsedTime(&m0, p->aev[0], p->aev[1]) != hipSuccess) { (void)hipGetLastError(); m0 = 0.f; }
    if (hipEventElapsedTime(&m1, p->aev[1], p->aev[2]) != hipSuccess) { (void)hipGetLastError(); m1 = 0.f; }
    p->ast.model_ms = m0;
    p->ast.resident_ms = c ? m1 : 0.0;
    p->ast.resident_bytes = c ? 16.0 * (double)S * (double)p->M + 8.0 * (double)p->M : 0.0;
    p->ast.column_from_chain = route;
    p->ast.appends += 1;
    // the object now describes gp2: it retains it and lets the old model go
    abo_retain(gp2);
    abo_gp* old = p->gp;
    p->gp = gp2;
    abo_destroy(old);
    p->N = N + 1; p->N4 = N4n; p->Xs = fv.Xs; p->st.N = p->N;
    return ABO_OK;
}

int32_t abo_paths_attach(void* paths, abo_cand* c) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p || !c) return fail(ABO_EINVAL, "abo_paths_attach: null argument");
    if (p->cset) return fail(ABO_EINVAL, "abo_paths_attach: a candidate set is attached already (one set per object: abo_paths_detach first)");
    if (cand_dim(c) != p->d) return fail(ABO_EDIM, "DimensionMismatch: candidate dimension %d, model dimension %d", cand_dim(c), p->d);
    if (cand_device(c) != p->dev) return fail(ABO_EINVAL, "abo_paths_attach: the candidate set lives on device %d, the model on %d", cand_device(c), p->dev);
    int32_t rc = check_model("abo_paths_attach", p);
    if (rc) return rc;
    PCHK(hipSetDevice(p->dev));
    hipStream_t s = gp_stream(p->gp);
    const int64_t M = cand_size(c), Mp = pad_up(M > 0 ? M : 1, RK_TILE), ntile = Mp / RK_TILE;
    const int S = p->S;
    size_t off = 0;
    const size_t o_g = take(off, sizeof(double) * S * Mp), o_c = take(off, sizeof(double) * Mp), o_k = take(off, sizeof(uint64_t) * S * ntile),
                 o_i = take(off, sizeof(int64_t) * S * ntile), o_tv = take(off, sizeof(double) * S), o_ti = take(off, sizeof(int64_t) * S);
    {
        const hipError_t e = scratch_alloc(p->dev, off, &p->gbuf, &p->gcap);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p->gbuf = nullptr; p->gcap = 0;
            return fail(ABO_ENOMEM, "abo_paths_attach: %zu bytes of resident path values: %s", off, hipGetErrorString(e));
        }
    }
    char* gb = static_cast<char*>(p->gbuf);
    p->G = reinterpret_cast<double*>(gb + o_g); p->ccol = reinterpret_cast<double*>(gb + o_c); p->pkey = reinterpret_cast<uint64_t*>(gb + o_k);
    p->pidx = reinterpret_cast<int64_t*>(gb + o_i); p->tv1 = reinterpret_cast<double*>(gb + o_tv); p->ti1 = reinterpret_cast<int64_t*>(gb + o_ti);
    p->cset = c; p->M = M; p->Mp = Mp; p->ntile = ntile;
    hipError_t e = hipMemsetAsync(p->G, 0, sizeof(double) * S * Mp, s);
    if (e != hipSuccess) { drop_resident(p); PCHK(e); }
    // the existing evaluation pass, values only and WITHOUT the exclusions: G holds g itself, the exclusions are read when it is used
    if (M > 0) {
        PathsEvalArgs a = eval_args(p);
        int64_t Mc = (int64_t)(PT_CHUNK_BYTES / (sizeof(double) * S)) / PT_CW * PT_CW;
        for (int64_t j0 = 0; j0 < M && e == hipSuccess; j0 += Mc) {
            a.Z = cand_points(c) + j0 * p->d; a.excl = nullptr; a.mc = std::min(Mc, M - j0);
            a.out_g = p->G + j0; a.ldg = Mp; a.out_neg = nullptr;
            e = launch_paths_eval(a, p->family, p->dp, p->NB, s);
        }
        if (e != hipSuccess) { (void)stream_wait(s); drop_resident(p); PCHK(e); }
    }
    rc = resident_select(p, nullptr, nullptr, s);
    if (!rc) { e = stream_wait(s); if (e != hipSuccess) rc = fail(ABO_EHIP, "abo_paths_attach: %s", hipGetErrorString(e)); }
    if (rc) { (void)stream_wait(s); drop_resident(p); return rc; }
    return ABO_OK;
}

int32_t abo_paths_detach(void* paths) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p) return fail(ABO_EINVAL, "abo_paths_detach: null paths object");
    if (!p->cset) return ABO_OK;
    PCHK(hipSetDevice(p->dev));
    PCHK(stream_wait(gp_stream(p->gp)));
    drop_resident(p);
    return ABO_OK;
}

int32_t abo_paths_values(void* paths, double* values, int32_t out_space) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p || !values) return fail(ABO_EINVAL, "abo_paths_values: null argument");
    if (out_space != ABO_HOST && out_space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_paths_values: unknown memory space %d", out_space);
    if (!p->cset) return fail(ABO_EINVAL, "abo_paths_values: no candidate set is attached (abo_paths_attach)");
    if (p->M == 0) return ABO_OK;
    PCHK(hipSetDevice(p->dev));
    hipStream_t s = gp_stream(p->gp);
    const int S = p->S;
    const int64_t M = p->M;
    Scratch sc(p->dev, s);
    double* out = values;
    if (out_space == ABO_HOST) { PCHK(sc.get(sizeof(double) * S * M)); out = sc.at<double>(0); }
    hipLaunchKernelGGL(paths_resident_copy_kernel, dim3(grid_for((int64_t)S * M)), dim3(256), 0, s, p->G, p->Mp, cand_mu(p->cset), M, S, 1.0, out, M);
    PCHK(hipGetLastError());
    if (out_space == ABO_HOST) PCHK(hipMemcpyAsync(values, out, sizeof(double) * S * M, hipMemcpyDeviceToHost, s));
    PCHK(stream_wait(s));
    return ABO_OK;
}

int32_t abo_paths_top(void* paths, int64_t idx_base, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p || !top_val || !top_idx) return fail(ABO_EINVAL, "abo_paths_top: null argument");
    if (k < 1) return fail(ABO_EINVAL, "abo_paths_top: k = %d", k);
    if (out_space != ABO_HOST && out_space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_paths_top: unknown memory space %d", out_space);
    if (!p->cset) return fail(ABO_EINVAL, "abo_paths_top: no candidate set is attached (abo_paths_attach)");
    PCHK(hipSetDevice(p->dev));
    hipStream_t s = gp_stream(p->gp);
    const int S = p->S;
    const int64_t M = p->M, n = (int64_t)S * k;
    const bool host = out_space == ABO_HOST;
    const int64_t we = k > 1 && M > 0 ? topk_workspace_entries(M, k) : 0;
    size_t off = 0;
    const size_t o_tv = take(off, host ? sizeof(double) * n : 0), o_ti = take(off, host ? sizeof(int64_t) * n : 0),
                 o_n = take(off, k > 1 ? sizeof(double) * (M > 0 ? M : 1) : 0), o_k0 = take(off, sizeof(uint64_t) * we),
                 o_k1 = take(off, sizeof(uint64_t) * we), o_i0 = take(off, sizeof(int64_t) * we), o_i1 = take(off, sizeof(int64_t) * we);
    Scratch sc(p->dev, s);
    PCHK(sc.get(off));
    double* tv = host ? sc.at<double>(o_tv) : top_val;
    int64_t* ti = host ? sc.at<int64_t>(o_ti) : top_idx;
    if (k == 1) {
        // what the fused reduction left after the last attach / append, unless the set's exclusions may have changed since
        CandSync cs{};
        cand_sync(p->cset, &cs);
        if (p->top_epoch != cs.mu_epoch) { const int32_t rc = resident_select(p, nullptr, nullptr, s); if (rc) return rc; }
        hipLaunchKernelGGL(paths_top1_emit_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, p->tv1, p->ti1, S, idx_base, tv, ti);
        PCHK(hipGetLastError());
    } else if (M == 0) {
        hipLaunchKernelGGL(paths_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tv, ti, n);
        PCHK(hipGetLastError());
    } else {
        TopkWork w{{sc.at<uint64_t>(o_k0), sc.at<uint64_t>(o_k1)}, {sc.at<int64_t>(o_i0), sc.at<int64_t>(o_i1)}};
        double* neg = sc.at<double>(o_n);
        for (int ps = 0; ps < S; ++ps) {
            hipLaunchKernelGGL(paths_resident_copy_kernel, dim3(grid_for(M)), dim3(256), 0, s, p->G + (int64_t)ps * p->Mp, p->Mp, cand_mu(p->cset), M, 1,
                               -1.0, neg, M);
            PCHK(hipGetLastError());
            PCHK(launch_topk(neg, M, k, idx_base, w, tv + (int64_t)ps * k, ti + (int64_t)ps * k, s));
        }
        hipLaunchKernelGGL(paths_negate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tv, ti, n);
        PCHK(hipGetLastError());
    }
    if (host) {
        PCHK(hipMemcpyAsync(top_val, tv, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        PCHK(hipMemcpyAsync(top_idx, ti, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
    }
    PCHK(stream_wait(s));
    return ABO_OK;
}

int32_t abo_paths_append_stats_get(void* paths, abo_paths_append_stats* out) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p || !out) return fail(ABO_EINVAL, "abo_paths_append_stats_get: null argument");
    *out = p->ast;
    return ABO_OK;
}

int32_t abo_paths_stats_get(void* paths, abo_paths_stats* out) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p || !out) return fail(ABO_EINVAL, "abo_paths_stats_get: null argument");
    *out = p->st;
    return ABO_OK;
}

}  // extern "C"
