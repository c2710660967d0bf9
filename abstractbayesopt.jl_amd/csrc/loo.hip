// Leave-one-out cross-validation from the resident W = L⁻¹ (Rasmussen & Williams §5.4.2): with B = K̃⁻¹ = WᵀW,
//     B_ii = Σ_{k ≥ i} W_ki²,   μ₋ᵢ = y_i − α_i/B_ii,   σ²₋ᵢ = 1/B_ii,
//     lpd_i = −½ log σ²₋ᵢ − (y_i − μ₋ᵢ)²/(2σ²₋ᵢ) − ½ log 2π,   nlpl = −Σ_i lpd_i
// — no refit and no K̃⁻¹ product: one read of the triangle of WT (row i of WT is column i of W, so the sum runs along a row, coalesced).
// The gradient of nlpl needs all of B and T = B·∂K/∂θ (api.hip forms them on the fp64 MFMA GEMM); the kernels here mirror B's lower
// 128-tiles into the upper ones and reduce the rows of T and B to the three partial derivatives.
// Every reduction runs in a fixed order (lane partials → butterfly → per-workgroup partial → one finishing workgroup): no atomics, the same
// bits on every call.
#include "abo_kernels.h"

namespace abo {

namespace {

constexpr int LOO_WAVES = 4;                     // waves per workgroup, one row (or one pair of rows) each

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Σ_{i ≤ k < N} WT[i][k]² over the wave's lanes: 16-byte loads from the 128-aligned start of the row's diagonal tile (k and k + 1 stay
// below the padded size, which the leading dimension covers), the entries left of the diagonal and right of N masked
__device__ __forceinline__ double row_sqnorm(const double* __restrict__ WT, int64_t ld, int i, int N, int lane) {
    const double* row = WT + (int64_t)i * ld;
    double acc = 0.0;
    for (int base = i & ~127; base < N; base += 128) {
        const int k = base + 2 * lane;
        const double2 v = *reinterpret_cast<const double2*>(row + k);
        if (k >= i && k < N) acc = fma(v.x, v.x, acc);
        if (k + 1 >= i && k + 1 < N) acc = fma(v.y, v.y, acc);
    }
    return wave_sum(acc);
}

// Row i's leave-one-out distribution from B_ii; returns lpd_i.  y_i − μ₋ᵢ = α_i/B_ii is used as it is (not as a difference of the two)
__device__ __forceinline__ double loo_epilogue(const LooArgs& p, int i, double bii) {
    const double var = 1.0 / bii;
    const double res = p.alpha[i] * var;
    const double y = p.delta[i] + p.mean_c;
    const double lpd = -0.5 * log(var) - 0.5 * res * res * bii - 0.91893853320467274178;   // ½ log 2π
    if (p.mu) p.mu[i] = y - res;
    if (p.var) p.var[i] = var;
    if (p.lpd) p.lpd[i] = lpd;
    return lpd;
}

// Workgroup b, wave w: row a = 4b + w from the top of the triangle and its mirror N − 1 − a from the bottom — N + 1 entries of WT per
// wave whatever b (row i has N − i), so the ragged triangle loads every workgroup alike.  partial[b] = Σ of the workgroup's ≤ 8 lpd_i.
__global__ void __launch_bounds__(64 * LOO_WAVES) loo_diag_kernel(LooArgs p) {
    __shared__ double part[LOO_WAVES][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = blockIdx.x * LOO_WAVES + wave, b = p.N - 1 - a;
    double l0 = 0.0, l1 = 0.0;
    if (a <= b) {
        const double s = row_sqnorm(p.WT, p.ld, a, p.N, lane);
        if (lane == 0) l0 = loo_epilogue(p, a, s);
    }
    if (a < b) {
        const double s = row_sqnorm(p.WT, p.ld, b, p.N, lane);
        if (lane == 0) l1 = loo_epilogue(p, b, s);
    }
    if (lane == 0) { part[wave][0] = l0; part[wave][1] = l1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < LOO_WAVES; ++w) s += part[w][0] + part[w][1];
        p.partial[blockIdx.x] = s;
    }
}

// out[q] = −Σ_b partial[b·nq + q] for q < nq ≤ 4: strided sums per thread, then a tree over the 256 threads
__global__ void __launch_bounds__(256) loo_finish_kernel(const double* __restrict__ partial, int nblocks, int nq, double* __restrict__ out) {
    __shared__ double r[4][256];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += 256)
        for (int q = 0; q < nq; ++q) s[q] += partial[(int64_t)b * nq + q];
    for (int q = 0; q < 4; ++q) r[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (threadIdx.x < o)
            for (int q = 0; q < 4; ++q) r[q][threadIdx.x] += r[q][threadIdx.x + o];
        __syncthreads();
    }
    if ((int)threadIdx.x < nq) out[threadIdx.x] = -r[threadIdx.x][0];
}

// B[i][j] = B[j][i] for every 128-tile above the diagonal (the K⁻¹ product writes the lower tiles, diagonal ones complete): 32×32 blocks
// through LDS, reads and writes both coalesced
__global__ void __launch_bounds__(256) loo_mirror_kernel(double* __restrict__ B, int64_t ld) {
    __shared__ double t[32][33];
    const int bi = blockIdx.y, bj = blockIdx.x;                  // 32-blocks: the destination is rows bi, columns bj
    if (bj / 4 <= bi / 4) return;
    const int x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
    for (int y = y0; y < 32; y += 8) t[y][x] = B[(int64_t)(bj * 32 + y) * ld + bi * 32 + x];
    __syncthreads();
    for (int y = y0; y < 32; y += 8) B[(int64_t)(bi * 32 + y) * ld + bj * 32 + x] = t[x][y];
}

// One wave per row i < N of T = B·D and B (both [Np][ld], complete): r_i = Σ_l T_il α_l, s_i = Σ_l T_il B_il, q_i = Σ_l B_il²,
// u_i = Σ_l B_il α_l over l < N, then with c = ½(1 + α_i²/B_ii) the row's terms of ∂(Σ lpd)/∂θ:
//     log ℓ      (α_i r_i − c s_i)/B_ii
//     log σ_f²   (α_i (α_i − σ² u_i) − c (B_ii − σ² q_i))/B_ii          (∂K = K̃ − σ²I:  B ∂K α = α − σ² Bα,  [B ∂K B]_ii = B_ii − σ² q_i)
//     log σ²     σ² (α_i u_i − c q_i)/B_ii                              (∂K = σ²I)
// partial[b·3 + θ] = Σ over the workgroup's four rows, in row order.
__global__ void __launch_bounds__(64 * LOO_WAVES) loo_grad_rows_kernel(LooGradArgs p) {
    __shared__ double part[LOO_WAVES][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * LOO_WAVES + wave;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (i < p.N) {
        const double* tr = p.T + (int64_t)i * p.ld;
        const double* br = p.B + (int64_t)i * p.ld;
        double r = 0.0, s = 0.0, q = 0.0, u = 0.0;
        for (int base = 0; base < p.N; base += 128) {
            const int l = base + 2 * lane;
            const double2 tv = *reinterpret_cast<const double2*>(tr + l);
            const double2 bv = *reinterpret_cast<const double2*>(br + l);
            const double2 av = *reinterpret_cast<const double2*>(p.alpha + l);
            if (l < p.N) { r = fma(tv.x, av.x, r); s = fma(tv.x, bv.x, s); q = fma(bv.x, bv.x, q); u = fma(bv.x, av.x, u); }
            if (l + 1 < p.N) { r = fma(tv.y, av.y, r); s = fma(tv.y, bv.y, s); q = fma(bv.y, bv.y, q); u = fma(bv.y, av.y, u); }
        }
        r = wave_sum(r); s = wave_sum(s); q = wave_sum(q); u = wave_sum(u);
        const double bii = br[i], ai = p.alpha[i], inv = 1.0 / bii;
        const double c = 0.5 * fma(ai * ai, inv, 1.0);
        g0 = (ai * r - c * s) * inv;
        g1 = (ai * (ai - p.noise * u) - c * (bii - p.noise * q)) * inv;
        g2 = p.noise * (ai * u - c * q) * inv;
    }
    if (lane == 0) { part[wave][0] = g0; part[wave][1] = g1; part[wave][2] = g2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < LOO_WAVES; ++w) v += part[w][threadIdx.x];
        p.partial[(int64_t)blockIdx.x * 3 + threadIdx.x] = v;
    }
}

}  // namespace

int loo_diag_blocks(int N) { return ((N + 1) / 2 + LOO_WAVES - 1) / LOO_WAVES; }
int loo_grad_blocks(int N) { return (N + LOO_WAVES - 1) / LOO_WAVES; }

hipError_t launch_loo_diag(const LooArgs& a, hipStream_t s) {
    const int nb = loo_diag_blocks(a.N);
    hipLaunchKernelGGL(loo_diag_kernel, dim3(nb), dim3(64 * LOO_WAVES), 0, s, a);
    hipLaunchKernelGGL(loo_finish_kernel, dim3(1), dim3(256), 0, s, a.partial, nb, 1, a.nlpl);
    return hipGetLastError();
}

hipError_t launch_loo_mirror(double* B, int64_t ld, int Np, hipStream_t s) {
    if (Np <= TB) return hipSuccess;                              // one tile: the diagonal tile is complete
    hipLaunchKernelGGL(loo_mirror_kernel, dim3(Np / 32, Np / 32), dim3(256), 0, s, B, ld);
    return hipGetLastError();
}

hipError_t launch_loo_grad_rows(const LooGradArgs& a, hipStream_t s) {
    const int nb = loo_grad_blocks(a.N);
    hipLaunchKernelGGL(loo_grad_rows_kernel, dim3(nb), dim3(64 * LOO_WAVES), 0, s, a);
    hipLaunchKernelGGL(loo_finish_kernel, dim3(1), dim3(256), 0, s, a.partial, nb, 3, a.out);
    return hipGetLastError();
}

}  // namespace abo
