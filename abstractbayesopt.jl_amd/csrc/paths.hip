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
    a.Xs = p->Xs; a.Wf = p->Wf; a.phase = p->phase; a.Btrain = p->B; a.Bfeat = p->B + p->N4 * p->Sp;
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
    if (p->buf) scratch_free(p->dev, p->buf, p->cap);
    if (p->gp) abo_destroy(p->gp);
    delete p;
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

int32_t abo_paths_stats_get(void* paths, abo_paths_stats* out) {
    abo_paths* p = static_cast<abo_paths*>(paths);
    if (!p || !out) return fail(ABO_EINVAL, "abo_paths_stats_get: null argument");
    *out = p->st;
    return ABO_OK;
}

}  // extern "C"
