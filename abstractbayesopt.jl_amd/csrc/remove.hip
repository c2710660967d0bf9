// abo_remove (include/abo_hip.h): the kernels that take observation j out of a fitted factor in O(N²) — DESIGN.md "Removing an
// observation".  With W = L⁻¹, ω = W[j][j], m = N − 1 − j trailing rows and
//   p_k = −W[j+1+k][j] / ω,   ρ_k² = 1 + Σ_{i<k} p_i²,   C = chol(I + ppᵀ)  (closed form in p and ρ)
// the new factor is  L′ = [[L11, 0], [L31, L33·C]]  and  W′ = [[W11, 0], [C⁻¹(W31 + p·W[j][:j]), C⁻¹·W33]]:
//   L′[r][k]  = L33[r][k]·ρ_{k+1}/ρ_k + p_k/(ρ_k ρ_{k+1}) · Σ_{k<i≤r} L33[r][i]·p_i          a SUFFIX scan along each row of L
//   W′[i][c]  = (ρ_i/ρ_{i+1})·M[i][c] − p_i/(ρ_i ρ_{i+1}) · Σ_{k<i} p_k·M[k][c]               a PREFIX scan down each column of W
// Both scans run along CONTIGUOUS memory: the first along the rows of L, the second along the rows of WT (= the columns of W), one
// wavefront per row, 256 elements per step (four coalesced 512-byte loads), the running sum carried in a register.  Rows are
// independent, so the N rows of a triangle keep every compute unit busy without a pass of partial sums.  W′ is then the tile
// transpose of WT′ (bit for bit, as after a fit).  The same walk over row c of WT accumulates B[c][j] = (WᵀW)[c][j], which the new
// α needs:  α′ = α − (α_j / B_jj)·B[:, j],  B_jj = ω²·ρ_m².
#include <hip/hip_runtime.h>

#include "abo_kernels.h"

namespace abo {
namespace {

constexpr int RM_WAVE = 64;
constexpr int RM_ROWS = 4;                       // rows (wavefronts) per workgroup
constexpr int RM_SUB = 4;                        // 64-element sub-blocks per scan step
constexpr int RM_STEP = RM_WAVE * RM_SUB;        // scan chunk: elements of one row per step (abo_kernels.h: REMOVE_SCAN_CHUNK)
static_assert(RM_STEP == REMOVE_SCAN_CHUNK, "the scan chunk the tests read");
constexpr int RM_PREP_THREADS = 1024;

// inclusive scan over the 64 lanes, in lane order (Hillis–Steele: the order tests/remove_oracle.py restates)
__device__ __forceinline__ double wave_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < RM_WAVE; o <<= 1) {
        const double t = __shfl_up(v, o, RM_WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = RM_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, RM_WAVE);
    return v;
}

// p, the scan coefficients and the row W[j][:j], from row j of WT and column j of WT.  One workgroup: the prefix sums ρ² are a scan
// over m ≤ N values (thread t owns a contiguous segment, the segment totals are scanned in LDS).
//   p[k], dl[k] = ρ_{k+1}/ρ_k, dw[k] = ρ_k/ρ_{k+1}, cc[k] = p_k/(ρ_k ρ_{k+1})  (k < m);  wj[c] = W[j][c]  (c < j)
//   scal = {ω, ρ_m², α_j}
__global__ void __launch_bounds__(RM_PREP_THREADS) remove_prep_kernel(const double* __restrict__ WT, int64_t ld, int N, int j,
                                                                      const double* __restrict__ alpha, double* __restrict__ p,
                                                                      double* __restrict__ dl, double* __restrict__ dw,
                                                                      double* __restrict__ cc, double* __restrict__ wj,
                                                                      double* __restrict__ scal) {
    __shared__ double seg[RM_PREP_THREADS];
    const int t = threadIdx.x;
    const int m = N - 1 - j;
    const double omega = WT[(int64_t)j * ld + j];
    const double* wrow = WT + (int64_t)j * ld + j + 1;            // W[j+1+k][j] = WT[j][j+1+k]
    const int per = (m + RM_PREP_THREADS - 1) / RM_PREP_THREADS;
    const int k0 = t * per, k1 = min(m, k0 + per);
    double acc = 0.0;
    for (int k = k0; k < k1; ++k) {
        const double pk = -wrow[k] / omega;
        p[k] = pk;
        acc += pk * pk;
    }
    seg[t] = acc;
    __syncthreads();
    for (int o = 1; o < RM_PREP_THREADS; o <<= 1) {               // inclusive scan of the segment totals
        const double add = t >= o ? seg[t - o] : 0.0;
        __syncthreads();
        seg[t] += add;
        __syncthreads();
    }
    double r2 = 1.0 + (t > 0 ? seg[t - 1] : 0.0);                 // ρ_{k0}²
    for (int k = k0; k < k1; ++k) {
        const double pk = p[k];
        const double r2n = r2 + pk * pk;
        const double rk = sqrt(r2), rn = sqrt(r2n);
        dl[k] = rn / rk;
        dw[k] = rk / rn;
        cc[k] = pk / (rk * rn);
        r2 = r2n;
    }
    for (int c = t; c < j; c += RM_PREP_THREADS) wj[c] = WT[(int64_t)c * ld + j];
    if (t == 0) {
        scal[0] = omega;
        scal[1] = 1.0 + seg[RM_PREP_THREADS - 1];
        scal[2] = alpha[j];
    }
}

// Row r′ of L′ (one wavefront): the part in front of column j is a copy; behind it the suffix scan.  Rows N′ ≤ r′ < Np′ are the
// identity padding.  Only the lower triangle is written (nothing reads the rest of the buffer abo_get_factor copies from).
__global__ void __launch_bounds__(RM_WAVE * RM_ROWS) remove_rows_L_kernel(const double* __restrict__ L, int64_t ld, double* __restrict__ Ln,
                                                                          int64_t ldn, int N, int Npn, int j,
                                                                          const double* __restrict__ p, const double* __restrict__ dl,
                                                                          const double* __restrict__ cc) {
    const int lane = threadIdx.x & (RM_WAVE - 1);
    const int rn = blockIdx.x * RM_ROWS + (threadIdx.x >> 6);     // new row
    if (rn >= Npn) return;
    double* out = Ln + (int64_t)rn * ldn;
    if (rn >= N - 1) {
        for (int c = lane; c < rn; c += RM_WAVE) out[c] = 0.0;
        if (lane == 0) out[rn] = 1.0;
        return;
    }
    const int r = rn + (rn >= j ? 1 : 0);                         // old row
    const double* in = L + (int64_t)r * ld;
    const int ncopy = min(j, rn + 1);
    for (int c = lane; c < ncopy; c += RM_WAVE) out[c] = in[c];
    if (r < j) return;
    const int kr = r - j - 1;                                     // last trailing column of this row
    const double* x33 = in + j + 1;
    double* o33 = out + j;
    double carry = 0.0;                                           // Σ over the columns to the right, already passed
    for (int base = 0; base <= kr; base += RM_STEP) {
        double x[RM_SUB], v[RM_SUB];
#pragma unroll
        for (int t = 0; t < RM_SUB; ++t) {
            const int k = kr - (base + t * RM_WAVE + lane);
            x[t] = k >= 0 ? x33[k] : 0.0;
            v[t] = k >= 0 ? x[t] * p[k] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < RM_SUB; ++t) {
            const int k = kr - (base + t * RM_WAVE + lane);
            const double inc = wave_scan(v[t], lane);
            double ex = __shfl_up(inc, 1, RM_WAVE);
            if (lane == 0) ex = 0.0;
            if (k >= 0) o33[k] = x[t] * dl[k] + cc[k] * (carry + ex);
            carry += __shfl(inc, RM_WAVE - 1, RM_WAVE);
        }
    }
}

// Row c′ of WT′ (one wavefront) over its full padded width: zeros in front of the diagonal, the copy of columns < j, the prefix scan
// behind them, zeros in the padding; rows N′ ≤ c′ < Np′ are rows of the identity.  The same walk sums Σ_k p_k·WT[c][j+1+k] for
// B[c][j] = ω·(W[j][c] − Σ), and writes α′[c′].
__global__ void __launch_bounds__(RM_WAVE * RM_ROWS) remove_rows_WT_kernel(const double* __restrict__ WT, int64_t ld, double* __restrict__ WTn,
                                                                           int64_t ldn, int N, int Npn, int j,
                                                                           const double* __restrict__ p, const double* __restrict__ dw,
                                                                           const double* __restrict__ cc, const double* __restrict__ wj,
                                                                           const double* __restrict__ scal,
                                                                           const double* __restrict__ alpha, double* __restrict__ alpha_n) {
    const int lane = threadIdx.x & (RM_WAVE - 1);
    const int cn = blockIdx.x * RM_ROWS + (threadIdx.x >> 6);     // new row of WT′ (= column of W′)
    if (cn >= Npn) return;
    double* out = WTn + (int64_t)cn * ldn;
    const int Nn = N - 1;
    if (cn >= Nn) {
        for (int c = lane; c < Npn; c += RM_WAVE) out[c] = c == cn ? 1.0 : 0.0;
        return;
    }
    const int c = cn + (cn >= j ? 1 : 0);                         // old row
    const double* in = WT + (int64_t)c * ld;
    for (int i = lane; i < cn; i += RM_WAVE) out[i] = 0.0;
    const int m = N - 1 - j;
    int kstart = 0;
    double w = 0.0;
    if (c < j) {
        for (int i = c + lane; i < j; i += RM_WAVE) out[i] = in[i];
        w = wj[c];
    } else {
        kstart = c - j - 1;
    }
    const double* x33 = in + j + 1;
    double* o33 = out + j;
    double carry = 0.0, sraw = 0.0;
    for (int base = kstart; base < m; base += RM_STEP) {
        double mv[RM_SUB], v[RM_SUB];
#pragma unroll
        for (int t = 0; t < RM_SUB; ++t) {
            const int k = base + t * RM_WAVE + lane;
            const double x = k < m ? x33[k] : 0.0;
            const double pk = k < m ? p[k] : 0.0;
            mv[t] = x + pk * w;
            v[t] = mv[t] * pk;
            sraw += x * pk;
        }
#pragma unroll
        for (int t = 0; t < RM_SUB; ++t) {
            const int k = base + t * RM_WAVE + lane;
            const double inc = wave_scan(v[t], lane);
            double ex = __shfl_up(inc, 1, RM_WAVE);
            if (lane == 0) ex = 0.0;
            if (k < m) o33[k] = dw[k] * mv[t] - cc[k] * (carry + ex);
            carry += __shfl(inc, RM_WAVE - 1, RM_WAVE);
        }
    }
    for (int i = Nn + lane; i < Npn; i += RM_WAVE) out[i] = 0.0;
    sraw = wave_sum(sraw);
    if (lane == 0) {
        const double omega = scal[0], rho2 = scal[1], aj = scal[2];
        alpha_n[cn] = alpha[c] - aj * (w - sraw) / (omega * rho2);   // (α_j / B_jj)·B[c][j], B_jj = ω²ρ_m², B[c][j] = ω(w − Σ)
    }
}

// W′ = WT′ᵀ over the Np′ × Np′ block, 32 × 32 tiles through LDS; tiles above the diagonal of W′ are zeros and read nothing
__global__ void __launch_bounds__(256) remove_transpose_kernel(const double* __restrict__ WT, double* __restrict__ W, int64_t ld) {
    __shared__ double tile[32][33];
    const int bx = blockIdx.x, by = blockIdx.y;                   // column tile and row tile of W′
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (bx > by) {
        for (int i = ty; i < 32; i += 8) W[(int64_t)(by * 32 + i) * ld + bx * 32 + tx] = 0.0;
        return;
    }
    for (int i = ty; i < 32; i += 8) tile[i][tx] = WT[(int64_t)(bx * 32 + i) * ld + by * 32 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8) W[(int64_t)(by * 32 + i) * ld + bx * 32 + tx] = tile[tx][i];
}

// index of the t-th kept point: t + #{removed indices in front of it}; idx sorted, b[q] = idx[q] − q is non-decreasing
__device__ __forceinline__ int64_t kept_source(const int64_t* __restrict__ idx, int k, int64_t t) {
    int lo = 0, hi = k;                                           // first q with idx[q] − q > t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idx[mid] - mid <= t) lo = mid + 1; else hi = mid;
    }
    return t + lo;
}

// the per-point arrays without the k points of idx (device, sorted): raw points, scaled points, targets, centred targets; a null
// destination is skipped
__global__ void __launch_bounds__(256) remove_gather_kernel(const int64_t* __restrict__ idx, int k, int64_t Nn, int d, int dp,
                                                            const double* __restrict__ Xraw, const double* __restrict__ Xs,
                                                            const double* __restrict__ y, const double* __restrict__ delta,
                                                            double* __restrict__ Xraw_n, double* __restrict__ Xs_n, double* __restrict__ y_n,
                                                            double* __restrict__ delta_n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < Nn; t += stride) {
        const int64_t src = kept_source(idx, k, t);
        for (int c = 0; c < d; ++c) Xraw_n[t * d + c] = Xraw[src * d + c];
        if (Xs_n) for (int c = 0; c < dp; ++c) Xs_n[t * dp + c] = Xs[src * dp + c];
        y_n[t] = y[src];
        if (delta_n) delta_n[t] = delta[src];
    }
}

}  // namespace

hipError_t launch_remove_row(const RemoveArgs& a, hipStream_t s) {
    const int Nn = a.N - 1;
    const int Npn = (int)pad_up(Nn, TB);
    if (a.N < 2 || a.j < 0 || a.j >= a.N || a.ld < a.N || a.ldn < Npn) return hipErrorInvalidValue;
    const int m = a.N - 1 - a.j;
    double* p = a.work;                                           // work: 4·m + j ≤ 5·N doubles
    double* dl = p + m;
    double* dw = dl + m;
    double* cc = dw + m;
    double* wj = cc + m;
    hipLaunchKernelGGL(remove_prep_kernel, dim3(1), dim3(RM_PREP_THREADS), 0, s, a.WT, a.ld, a.N, a.j, a.alpha, p, dl, dw, cc, wj, a.scal);
    const unsigned rows = (unsigned)((Npn + RM_ROWS - 1) / RM_ROWS);
    hipLaunchKernelGGL(remove_rows_L_kernel, dim3(rows), dim3(RM_WAVE * RM_ROWS), 0, s, a.L, a.ld, a.Ln, a.ldn, a.N, Npn, a.j, p, dl, cc);
    hipLaunchKernelGGL(remove_rows_WT_kernel, dim3(rows), dim3(RM_WAVE * RM_ROWS), 0, s, a.WT, a.ld, a.WTn, a.ldn, a.N, Npn, a.j, p, dw, cc,
                       wj, a.scal, a.alpha, a.alpha_n);
    hipLaunchKernelGGL(remove_transpose_kernel, dim3(Npn / 32, Npn / 32), dim3(256), 0, s, a.WTn, a.Wn, a.ldn);
    return hipGetLastError();
}

hipError_t launch_remove_gather(const int64_t* idx, int k, int64_t Nn, int d, int dp, const double* Xraw, const double* Xs, const double* y,
                                const double* delta, double* Xraw_n, double* Xs_n, double* y_n, double* delta_n, hipStream_t s) {
    if (Nn < 1 || k < 1) return hipErrorInvalidValue;
    int64_t blocks = (Nn + 255) / 256;
    blocks = blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(remove_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, idx, k, Nn, d, dp, Xraw, Xs, y, delta, Xraw_n, Xs_n,
                       y_n, delta_n);
    return hipGetLastError();
}

}  // namespace abo
