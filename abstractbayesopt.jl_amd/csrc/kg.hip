// Knowledge gradient over a discrete decision set (abo_acq_kg; api.hip drives it):
//     KG_i = E[max_j (a_j + b_ij·Z)] − max_j a_j,   Z ~ N(0, 1),   a_j = −μ(zb_j),   b_ij = cov(f(za_i), f(zb_j))/sqrt(v_i + σ_n²)
// evaluated exactly (Frazier, Powell and Dayanik 2009, Algorithm 1): the lines of a row sorted by (b, a), of equal slopes the largest
// intercept kept, one stack scan for the upper envelope e_0 … e_m with its breakpoints c_1 … c_m, and
//     KG = Σ_t (b_{e_t} − b_{e_{t−1}})·h(−|c_t|),   h(z) = φ(z) + z·Φ(z),   Φ(z) = ½·erfc(−z/√2) at z ≤ 0 — every term ≥ 0.
// One workgroup owns one row of the padded covariance block and keeps its lines in LDS from the load to the sum; nothing of the block
// leaves the device.  No atomics: every output has one writer, and the terms are summed in envelope order by one lane — the same bits
// on every call.
#include "abo_kernels.h"

namespace abo {

namespace {

constexpr int KG_THREADS = 256;
constexpr double KG_VAR_FLOOR = 1e-12;           // v_i + σ_n² at or below it: the row is 0.0 (the σ² ≤ 1e-12 branch of the EI / PI epilogues)

__device__ __forceinline__ bool kg_less(const double2 p, const double2 q) { return p.x < q.x || (p.x == q.x && p.y < q.y); }

// h(z) = φ(z) + z·Φ(z) at z ≤ 0.  Φ underflows before φ·(1/|z|) does not matter: where Φ is 0 the product is taken as 0 (z = −Inf, a
// breakpoint that overflowed, would give −Inf·0 otherwise)
__device__ __forceinline__ double kg_h(double z) {
    const double Phi = 0.5 * erfc(-z * 0.70710678118654752440);
    return 0.39894228040143267794 * exp(-0.5 * z * z) + (Phi == 0.0 ? 0.0 : z * Phi);
}

// Row i = blockIdx.x.  LDS (dynamic, 16-byte aligned, no static beside it): slot[0 … P] of (b, a) pairs, then two ints {non-finite
// flag, m}.  The lines are loaded into and sorted in slot[1 … P] (P = the power of two ≥ Mb; the padding is (+Inf, +Inf) and sorts
// behind every line); the envelope stack grows from slot[0]: with the row's own line merged in from a register it holds at most one
// entry more than the lines read so far, so its top never reaches an unread slot.
__global__ void __launch_bounds__(KG_THREADS) kg_row_kernel(KgArgs g) {
    extern __shared__ __attribute__((aligned(16))) char kg_lds[];
    double2* slot = reinterpret_cast<double2*>(kg_lds);
    double2* line = slot + 1;
    int* word = reinterpret_cast<int*>(slot + g.P + 1);
    const int t = threadIdx.x, i = blockIdx.x;
    const int Mb = g.Mb, P = g.P;
    const double den = g.den ? g.den[i] : 1.0;
    if (den == 0.0) {                                         // (uniform over the workgroup)
        if (t == 0) { g.val[i] = 0.0; if (g.nenv) g.nenv[i] = 1; }
        return;
    }
    const bool has_self = g.self_b != nullptr;
    double2 self = make_double2(0.0, 0.0);
    if (has_self) self = make_double2(g.self_b[i], g.asign * g.self_a[i]);
    if (t == 0) { word[0] = (isfinite(self.x) && isfinite(self.y)) ? 0 : 1; word[1] = 0; }
    __syncthreads();
    const double* Bi = g.B + (int64_t)i * g.ldb;
    bool bad = false;
    for (int j = t; j < P; j += KG_THREADS) {
        double2 v = make_double2(INFINITY, INFINITY);
        if (j < Mb) {
            v = make_double2(Bi[j] / den, g.asign * g.a[j]);
            bad = bad || !(isfinite(v.x) && isfinite(v.y));
        }
        line[j] = v;
    }
    if (bad) word[0] = 1;                                     // (every writer stores the same value)
    __syncthreads();
    if (word[0]) {
        if (t == 0) { g.val[i] = NAN; if (g.nenv) g.nenv[i] = 0; }
        return;
    }
    // bitonic sort of line[0 … P) by (b, a) ascending
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = t; e < (P >> 1); e += KG_THREADS) {
                const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo + j;
                const double2 x = line[lo], y = line[hi];
                const bool up = (lo & k) == 0;
                if (up ? kg_less(y, x) : kg_less(x, y)) { line[lo] = y; line[hi] = x; }
            }
            __syncthreads();
        }
    }
    // the envelope: one lane, in place.  A line of the top's slope replaces the top (it comes later in the order: its intercept is
    // the larger one); a line whose breakpoint with the top is not beyond the breakpoint under the top pops the top.
    if (t == 0) {
        int top = -1, r = 0;
        bool pending = has_self;
        while (r < Mb || pending) {
            double2 ln;
            if (pending && (r >= Mb || kg_less(self, line[r]))) { ln = self; pending = false; }
            else ln = line[r++];
            while (top >= 0) {
                const double2 tp = slot[top];
                if (ln.x == tp.x) { --top; continue; }
                if (top == 0) break;
                const double2 ud = slot[top - 1];
                const double c_new = (tp.y - ln.y) / (ln.x - tp.x), c_top = (ud.y - tp.y) / (tp.x - ud.x);
                if (c_new <= c_top) --top; else break;
            }
            slot[++top] = ln;
        }
        word[1] = top;
    }
    __syncthreads();
    const int m = word[1];
    // the m terms, 256 at a time from the top down: term t reads slots t − 1 and t and lands in slot t, which no later round reads
    for (int hi = m; hi >= 1; hi -= KG_THREADS) {
        const int tt = hi - t;
        double term = 0.0;
        if (tt >= 1) {
            const double2 p = slot[tt - 1], q = slot[tt];
            const double db = q.x - p.x, c = (p.y - q.y) / db;
            term = db * kg_h(-fabs(c));
        }
        __syncthreads();
        if (tt >= 1) slot[tt].x = term;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int e = 1; e <= m; ++e) s += slot[e].x;          // envelope order: one order, one set of bits
        g.val[i] = s;
        if (g.nenv) g.nenv[i] = m + 1;
    }
}

// Per candidate i, one wave: v_i = C[i][i] (the symmetric form's diagonal) or σ_f² − Σ_k V[i][k]² (the rectangular form: lanes stride the
// row, one shuffle tree — a fixed order), both + 1e-18 as abo_predict's variance carries it; den[i] = sqrt(v_i + noise), 0 where that
// sum is ≤ 1e-12 (the row's KG is then 0.0); self_b[i] = v_i/den[i], the slope of the candidate's own line.
__global__ void __launch_bounds__(256) kg_prep_kernel(const double* __restrict__ V, int64_t ldv, int R, const double* __restrict__ C,
                                                      int64_t ldc, int Ma, double sigma_f2, double noise, double* __restrict__ den,
                                                      double* __restrict__ self_b) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Ma) return;
    double v;
    if (C) {
        v = C[(int64_t)i * ldc + i];
    } else {
        const double* Vi = V + (int64_t)i * ldv;
        double s = 0.0;
        for (int k = lane; k < R; k += 64) s = fma(Vi[k], Vi[k], s);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        v = sigma_f2 - s;
    }
    v += 1e-18;
    if (lane == 0) {
        const double x = v + noise;
        const double dn = x <= KG_VAR_FLOOR ? 0.0 : sqrt(x);
        den[i] = dn;
        self_b[i] = dn == 0.0 ? 0.0 : v / dn;
    }
}

}  // namespace

size_t kg_lds_bytes(int Mb) { return sizeof(double) * 2 * ((size_t)kg_pow2(Mb) + 1) + 16; }

hipError_t launch_kg_rows(KgArgs a, hipStream_t s) {
    if (a.Ma <= 0) return hipSuccess;
    if (a.Mb < 1 || a.Mb > KG_MAX_LINES || !a.a || !a.B || !a.val || (a.self_b && !a.self_a)) return hipErrorInvalidValue;
    a.P = kg_pow2(a.Mb);
    const size_t lds = kg_lds_bytes(a.Mb);
    if (lds > 64 * 1024) {
        // beyond the default cap of dynamic LDS (Mb > 2048; 128 KiB + 32 B at 8192).  Function attributes are per device, so the cap is
        // raised on the device this launch goes to, every time: a host call of microseconds in front of a kernel of milliseconds
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kg_row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)kg_lds_bytes(KG_MAX_LINES));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kg_row_kernel, dim3((unsigned)a.Ma), dim3(KG_THREADS), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_kg_prep(const double* V, int64_t ldv, int R, const double* C, int64_t ldc, int Ma, double sigma_f2, double noise,
                          double* den, double* self_b, hipStream_t s) {
    if (Ma <= 0) return hipSuccess;
    hipLaunchKernelGGL(kg_prep_kernel, dim3((unsigned)((Ma + 3) / 4)), dim3(256), 0, s, V, ldv, R, C, ldc, Ma, sigma_f2, noise, den, self_b);
    return hipGetLastError();
}

}  // namespace abo
