// Monte-Carlo joint q-EI on a resident candidate set (include/abo_hip.h: abo_cand_qei_mc; SURVEY.md §8 a13 (iii), the second definition
// of q-EI: "a Monte-Carlo joint q-EI over Σ_q = K_qq − V_qᵀV_q").  No reference counterpart: the reference's EI is single-point
// (src/acquisition_functions/ExpectedImprovement.jl:40-66), which this tends to at q = 1 and S → ∞.
//
// The batch is chosen greedily, one point at a time, on the machinery of the Kriging-believer block form (qei.hip): Cov₀ columns of a
// block of T points from ONE pass over the resident K_ZX, and the rank-1 chain — here with NOISE-FREE pivots,
//     c_i(z) = Cov(z, x_i) − Σ_{k<i} c_k(z)·c_k(x_i)/s_k,   v_i(z) = v_{i−1}(z) − c_i(z)²/s_i,   s_i = v_{i−1}(x_i),   v_0 = σ²
// (s_i ≤ 1e-12: a zero column).  Conditioned jointly on the LATENT values, h_i(z) = c_i(z)/√s_i is row z of the Cholesky factor of the
// joint covariance of (f(x_1), …, f(x_{j−1}), f(z)) and √v_{j−1}(z) its diagonal, so with the caller's base samples ζ (S × q)
//     F^s_j(z) = μ(z) + Σ_{i<j} h_i(z)·ζ[s][i−1] + σ_j(z)·ζ[s][j−1]          (σ_j = √v_{j−1} if v_{j−1} > 1e-12, else 0)
//     R^s_j = max(R^s_{j−1}, best_y − ξ − F^s_j(x_j)),  R^s_0 = 0;    qEI_j(z) = (1/S)·Σ_s max(R^s_{j−1}, best_y − ξ − F^s_j(z))
//
// qei_mc_step_kernel<NK>: launch k (k = 0 … q) finishes pick k − 1 and selects pick k, as qei_step_kernel does for the KB batch:
//   (B) every workgroup reduces the partial arg-maxima of launch k − 1, looks the winner up in the slot table, forms the chain entry
//       c_k = C₀[slot] − Σ_real γ_i c_i − Σ_batch γ_m c_m with the noise-free pivot, v −= c²/s, and R^s_k from the pick's own sample
//       vector (every workgroup recomputes it from the pick's μ, v and chain values — the arithmetic the pick's lane scored it with);
//   (C) scores its candidates, one per lane: the coefficients (h_1 … h_k, σ) stay in registers (NK ≥ k + 1, a power of two, zeros
//       behind), ζ and R are staged in LDS tiles of QMC_TS samples (static: ≤ 34 KiB at NK = 32) and read as broadcasts.  The scores go
//       to a [M] buffer: a pick outside every block raises st->stop and the host builds a block around the top T of them.
// Only R[S] (and the partials) cross launches; no workgroup waits for another inside a launch, no global atomics: bit-reproducible.
// The set's stored (μ, σ²) and its chain are only read; the batch's own chain entries and variances live in scratch of the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/abo_hip.h"
#include "abo_acq_dev.h"
#include "abo_internal.h"
#include "abo_kernels.h"

namespace abo {
namespace {

constexpr int QMC_MAXQ = 32;                 // picks of one batch
constexpr int QMC_MAXS = 4096;               // base samples
constexpr int QMC_TS = 128;                  // samples per LDS tile
constexpr int QMC_MAXWG = QEI_STEP_MAXWG;
constexpr uint64_t QMC_KEY_PAD = 0ull;
constexpr int64_t QMC_IDX_PAD = 0x7fffffffffffffffll;
constexpr double QMC_TINY = 1e-12;           // the EI threshold of the reference (ExpectedImprovement.jl:59)

struct QmcState {                            // device memory, one per call
    int32_t stop;                            // 0: running; 1: pick stop_at is in no block; 3: no candidate left for pick stop_at
    int32_t stop_at;
    double s[QMC_MAXQ];                      // noise-free pivot of pick t (≤ QMC_TINY: a zero column)
    int64_t pick[QMC_MAXQ];                  // local index of pick t
};

struct QmcArgs {
    const double* mu; const double* var;     // [M] stored posterior of the set (read only)
    double* v;                               // [M] v_k(z) of this batch (launch 0 copies σ²)
    const double* Z;                         // [M][d]
    const double* blk;                       // [slots][Mp] block columns
    const double* chain;                     // the set's chain; rows [0, nreal) are its real entries (noisy pivots real_s)
    double* bc;                              // [q − 1][Mp] the batch's entries c_1 … c_{q−1}
    const double* base;                      // [S][q] base samples
    double* R;                               // [2][S]: launch k writes half k & 1, reads half (k − 1) & 1
    double* score;                           // [M] qEI of every candidate for the launch's pick (−Inf: not eligible)
    QmcState* st;
    QeiStepPartial* part;                    // [2][QMC_MAXWG]: launch k writes half k & 1, reads half (k − 1) & 1
    double* rec;                             // [q][4 + d] {qEI, global index, μ, v, x[d]}
    int64_t M, Mp, idx_base;
    int d, T16, nslots, k, q, S, nreal, nwg_prev;
    double xi, best_y;
    double real_s[QEI_MAXQ];
    int blk_base[4];
    int64_t slot_gidx[4 * QEI_MAXT];
};

__device__ __forceinline__ void mc_wg_argmax(uint64_t& bk, int64_t& bi, double& bm, double& bv, uint64_t* sk, int64_t* si, double* sm,
                                             double* sv) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t ok = (uint64_t)__shfl_xor((long long)bk, o);
        const int64_t oi = (int64_t)__shfl_xor((long long)bi, o);
        const double om = __shfl_xor(bm, o), ov = __shfl_xor(bv, o);
        if (before(ok, oi, bk, bi)) { bk = ok; bi = oi; bm = om; bv = ov; }
    }
    if (lane == 0) { sk[wave] = bk; si[wave] = bi; sm[wave] = bm; sv[wave] = bv; }
    __syncthreads();
    bk = sk[0]; bi = si[0]; bm = sm[0]; bv = sv[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (before(sk[w], si[w], bk, bi)) { bk = sk[w]; bi = si[w]; bm = sm[w]; bv = sv[w]; }
    __syncthreads();
}

template <int NK>
__global__ void __launch_bounds__(256) qei_mc_step_kernel(const QmcArgs a) {
    __shared__ uint64_t sk[4];
    __shared__ int64_t si[4];
    __shared__ double sm[4], sv[4];
    __shared__ double gam[QEI_MAXQ + QMC_MAXQ];  // γ of the real entries [0, nreal), then of the batch's entries from QEI_MAXQ on
    __shared__ double rs[QMC_MAXQ];              // 1/√s of the batch's entries (0: a zero column)
    __shared__ double gw[NK];                    // the pick's coefficients (h_1(x) … h_{k−1}(x), σ(x), zeros)
    __shared__ int64_t picked[QMC_MAXQ];
    __shared__ int s_slot;
    __shared__ double zt[QMC_TS * NK];           // ζ[s][0 … NK) of a tile (columns > k are zero)
    __shared__ double rt[QMC_TS];                // R^s of the tile
    const int t = threadIdx.x, k = a.k;
    if (t == 0) s_slot = a.st->stop;             // an earlier launch of the batch asked for the host: read ONCE per workgroup (workgroup 0
    __syncthreads();                             // of this launch may raise it meanwhile), so that all waves return or none
    if (s_slot) return;
    const int nb = k > 0 ? k - 1 : 0;            // the batch's chain entries before this launch's
    int first = 0, slot = -1;
    bool zero = false;
    double piv = 1.0, uw = 0.0;
    if (k > 0) {
        // (B) the winner of launch k − 1: pick k − 1
        const QeiStepPartial* pp = a.part + (size_t)((k - 1) & 1) * QMC_MAXWG;
        uint64_t bk = QMC_KEY_PAD;
        int64_t bi = QMC_IDX_PAD;
        double bm = 0.0, bv = 0.0;
        for (int e = t; e < a.nwg_prev; e += 256) {
            const QeiStepPartial p = pp[e];
            if (before(p.key, p.idx, bk, bi)) { bk = p.key; bi = p.idx; bm = p.mu; bv = p.var; }
        }
        mc_wg_argmax(bk, bi, bm, bv, sk, si, sm, sv);
        if (bi == QMC_IDX_PAD) {                 // every candidate is excluded or picked already
            if (blockIdx.x == 0 && t == 0) { a.st->stop_at = k - 1; a.st->stop = 3; }
            return;
        }
        const int64_t li = bi, gidx = li + a.idx_base;
        if (blockIdx.x == 0) {
            double* r = a.rec + (size_t)(k - 1) * (4 + a.d);
            if (t == 0) { r[0] = score_of_key(bk); r[1] = (double)gidx; r[2] = bm; r[3] = bv; a.st->pick[k - 1] = li; }
            for (int c = t; c < a.d; c += 256) r[4 + c] = a.Z[li * a.d + c];
        }
        if (k == a.q) return;                    // the tail launch: the last pick conditions nothing
        if (t == 0) s_slot = 0x7fffffff;
        __syncthreads();
        for (int e = t; e < a.nslots; e += 256)  // the pick's block row: the FIRST slot holding its index
            if (a.slot_gidx[e] == gidx) atomicMin(&s_slot, e);
        for (int i = t; i < a.nreal; i += 256) gam[i] = a.chain[(int64_t)i * a.Mp + li] / a.real_s[i];
        if (t < k) {                             // (one thread per batch entry: rs[t] is its own)
            const double s_t = t < nb ? a.st->s[t] : bv;
            rs[t] = s_t > QMC_TINY ? 1.0 / sqrt(s_t) : 0.0;
            picked[t] = t < nb ? a.st->pick[t] : li;
            if (t < nb) gam[QEI_MAXQ + t] = s_t > QMC_TINY ? a.bc[(int64_t)t * a.Mp + li] / s_t : 0.0;
        }
        if (t < NK)                              // as the pick's lane formed its coefficients in launch k − 1
            gw[t] = t < nb ? a.bc[(int64_t)t * a.Mp + li] * (a.st->s[t] > QMC_TINY ? 1.0 / sqrt(a.st->s[t]) : 0.0)
                           : (t == nb && bv > QMC_TINY ? sqrt(bv) : 0.0);
        __syncthreads();
        slot = s_slot == 0x7fffffff ? -1 : s_slot;
        if (slot < 0) {
            if (blockIdx.x == 0 && t == 0) { a.st->stop_at = k - 1; a.st->stop = 1; }
            return;
        }
        if (blockIdx.x == 0 && t == 0) a.st->s[k - 1] = bv;
        first = a.blk_base[slot / a.T16];        // entries before it are already in the block's columns
        piv = bv;
        zero = !(bv > QMC_TINY);
        uw = (a.best_y - a.xi) - bm;
    }
    const double* blk = a.blk + (int64_t)(slot < 0 ? 0 : slot) * a.Mp;
    double* out = a.bc + (int64_t)nb * a.Mp;
    const double* Rprev = a.R + (size_t)((k + 1) & 1) * a.S;
    double* Rnext = a.R + (size_t)(k & 1) * a.S;
    const double u0 = a.best_y - a.xi;
    uint64_t bk = QMC_KEY_PAD;
    int64_t bi = QMC_IDX_PAD;
    double bm = 0.0, bv = 0.0;
    bool first_chunk = true;
    for (int64_t z0 = (int64_t)blockIdx.x * 256; z0 < a.M; z0 += (int64_t)gridDim.x * 256, first_chunk = false) {
        const int64_t z = z0 + t;
        const bool act = z < a.M;
        double m = 0.0, v = 0.0;
        double g[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) g[i] = 0.0;
        bool elig = false;
        if (act) {
            m = a.mu[z];
            v = k == 0 ? a.var[z] : a.v[z];
            if (k > 0) {
                double c = blk[z];
                for (int i = first; i < a.nreal; ++i) c = fma(-gam[i], a.chain[(int64_t)i * a.Mp + z], c);  // fixed order: real entries,
#pragma unroll
                for (int i = 0; i < NK; ++i)                                                                  // then the batch's
                    if (i < nb) {
                        const double ci = a.bc[(int64_t)i * a.Mp + z];
                        c = fma(-gam[QEI_MAXQ + i], ci, c);
                        g[i] = ci * rs[i];
                    }
                if (zero) c = 0.0;
                out[z] = c;
                if (!zero) v = v - c * c / piv;  // the expression of qei_step_kernel
#pragma unroll
                for (int i = 0; i < NK; ++i)
                    if (i == nb) g[i] = c * rs[nb];
            }
            a.v[z] = v;
            const double sg = v > QMC_TINY ? sqrt(v) : 0.0;
#pragma unroll
            for (int i = 0; i < NK; ++i)
                if (i == k) g[i] = sg;
            elig = m != HUGE_VAL;                // abo_cand_exclude: μ = +Inf
            for (int i = 0; i < k; ++i) elig = elig && picked[i] != z;
        }
        double acc = 0.0;
        const double u = u0 - m;
        for (int s0 = 0; s0 < a.S; s0 += QMC_TS) {
            const int ns = min(QMC_TS, a.S - s0);
            __syncthreads();                     // the previous tile is consumed
            for (int e = t; e < QMC_TS * NK; e += 256) {
                const int r = e / NK, col = e % NK;
                zt[e] = (r < ns && col <= k) ? a.base[(int64_t)(s0 + r) * a.q + col] : 0.0;
            }
            __syncthreads();
            if (t < ns) {                        // R^s_k = max(R^s_{k−1}, best_y − ξ − F^s(x_{k−1}))
                double r = 0.0;
                if (k > 0) {
                    double im = uw;
#pragma unroll
                    for (int i = 0; i < NK; ++i) im = fma(-gw[i], zt[t * NK + i], im);
                    r = fmax(Rprev[s0 + t], im);
                }
                rt[t] = r;
                if (blockIdx.x == 0 && first_chunk) Rnext[s0 + t] = r;
            }
            __syncthreads();
            if (elig)
                for (int r = 0; r < ns; ++r) {
                    double im = u;
#pragma unroll
                    for (int i = 0; i < NK; ++i) im = fma(-g[i], zt[r * NK + i], im);
                    acc += fmax(rt[r], im);
                }
        }
        const double sc = elig ? acc / (double)a.S : -HUGE_VAL;
        if (act) a.score[z] = sc;
        if (elig) {
            const uint64_t key = score_key(sc);
            if (before(key, z, bk, bi)) { bk = key; bi = z; bm = m; bv = v; }
        }
    }
    mc_wg_argmax(bk, bi, bm, bv, sk, si, sm, sv);
    if (t == 0) {
        QeiStepPartial p;
        p.key = bk; p.idx = bi; p.mu = bm; p.var = bv;
        a.part[(size_t)(k & 1) * QMC_MAXWG + blockIdx.x] = p;
    }
}

template <int NK>
hipError_t launch_nk(const QmcArgs& a, int nwg, hipStream_t s) {
    hipLaunchKernelGGL(qei_mc_step_kernel<NK>, dim3((unsigned)nwg), dim3(256), 0, s, a);
    return hipGetLastError();
}

// launch k scores with k + 1 coefficients (the tail launch k = q scores nothing)
hipError_t launch_qei_mc_step(const QmcArgs& a, int nwg, hipStream_t s) {
    if (nwg < 1 || nwg > QMC_MAXWG || a.M < 1 || a.q < 1 || a.q > QMC_MAXQ || a.k < 0 || a.k > a.q || a.S < 1 || a.S > QMC_MAXS)
        return hipErrorInvalidValue;
    const int need = a.k + 1;
    if (need <= 2) return launch_nk<2>(a, nwg, s);
    if (need <= 4) return launch_nk<4>(a, nwg, s);
    if (need <= 8) return launch_nk<8>(a, nwg, s);
    if (need <= 16) return launch_nk<16>(a, nwg, s);
    return launch_nk<32>(a, nwg, s);
}

int32_t fail(int32_t code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return set_error(code, buf);
}

size_t take(size_t& off, size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
}

// The batch on the open block state (scratch of the call: `buf`).  rc != 0: the reason is in the last error.
int32_t qei_mc_drive(abo_gp* g, abo_cand* c, int q, double xi, double best_y, const double* base, int S, int32_t base_space,
                     int64_t idx_base, int T, double* x_out, int64_t* idx_out, double* qei_out) {
    QeiMcView V{};
    qei_mc_view(c, &V);
    hipStream_t s = gp_stream(g);
    const int dev = gp_device(g), d = V.d, wrec = 4 + d;
    const int64_t M = V.M;
    const int Tk = (int)std::min<int64_t>(T, M);
    const int64_t we = topk_workspace_entries(M, Tk);
    size_t off = 0;
    const size_t o_st = take(off, sizeof(QmcState)), o_part = take(off, sizeof(QeiStepPartial) * 2 * QMC_MAXWG),
                 o_rec = take(off, sizeof(double) * q * wrec), o_R = take(off, sizeof(double) * 2 * S),
                 o_base = take(off, base_space == ABO_HOST ? sizeof(double) * S * q : 0), o_v = take(off, sizeof(double) * M),
                 o_sc = take(off, sizeof(double) * M), o_bc = take(off, sizeof(double) * (q > 1 ? q - 1 : 1) * V.Mp),
                 o_k0 = take(off, sizeof(uint64_t) * we), o_k1 = take(off, sizeof(uint64_t) * we), o_i0 = take(off, sizeof(int64_t) * we),
                 o_i1 = take(off, sizeof(int64_t) * we), o_tv = take(off, sizeof(double) * Tk), o_ti = take(off, sizeof(int64_t) * Tk),
                 o_pts = take(off, sizeof(double) * Tk * d);
    void* buf = nullptr;
    size_t cap = 0;
    hipError_t e = scratch_alloc(dev, off, &buf, &cap);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "abo_cand_qei_mc: scratch allocation failed");
    struct Release { int dev; void* p; size_t cap; hipStream_t s; ~Release() { (void)stream_wait(s); scratch_free(dev, p, cap); } }
        release{dev, buf, cap, s};
    char* b = static_cast<char*>(buf);
    QmcArgs a{};
    a.mu = V.mu; a.var = V.var; a.v = reinterpret_cast<double*>(b + o_v); a.Z = V.Z; a.chain = V.chain;
    a.bc = reinterpret_cast<double*>(b + o_bc);
    a.base = base_space == ABO_HOST ? reinterpret_cast<const double*>(b + o_base) : base;
    a.R = reinterpret_cast<double*>(b + o_R); a.score = reinterpret_cast<double*>(b + o_sc);
    a.st = reinterpret_cast<QmcState*>(b + o_st); a.part = reinterpret_cast<QeiStepPartial*>(b + o_part);
    a.rec = reinterpret_cast<double*>(b + o_rec);
    a.M = M; a.Mp = V.Mp; a.idx_base = idx_base; a.d = d; a.q = q; a.S = S; a.xi = xi; a.best_y = best_y;
    a.nreal = V.nreal;
    for (int i = 0; i < V.nreal; ++i) a.real_s[i] = V.chain_s[i];
    const int nwg = (int)std::min<int64_t>((M + 255) / 256, QMC_MAXWG);
    a.nwg_prev = nwg;
    if (base_space == ABO_HOST) e = hipMemcpyAsync(b + o_base, base, sizeof(double) * S * q, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(a.st, 0, sizeof(QmcState), s);
    std::vector<double> rec((size_t)q * wrec), pts((size_t)Tk * d);
    std::vector<int64_t> gix(Tk);
    QmcState hst{};
    int k_from = 0;
    while (e == hipSuccess) {
        a.blk = V.blk; a.T16 = V.T16; a.nslots = V.nslots;
        for (int i = 0; i < 4; ++i) a.blk_base[i] = i < V.nslots / V.T16 ? V.blk_base[i] : 0;
        for (int i = 0; i < 4 * QEI_MAXT; ++i) a.slot_gidx[i] = i < V.nslots ? V.slot_gidx[i] : -1;
        for (int k = k_from; k <= q && e == hipSuccess; ++k) { a.k = k; e = launch_qei_mc_step(a, nwg, s); }
        if (e == hipSuccess) e = hipMemcpyAsync(&hst, a.st, sizeof(QmcState), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(rec.data(), a.rec, sizeof(double) * rec.size(), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = stream_wait(s);
        if (e != hipSuccess || !hst.stop) break;
        if (hst.stop == 3)
            return fail(ABO_EINVAL, "abo_cand_qei_mc: no candidate left for pick %d (the set holds fewer than q that are not excluded)",
                        hst.stop_at + 1);
        // pick stop_at lies in no block: a new block around the scores that selected it, then the launches from stop_at + 1 again
        const int64_t gpick = (int64_t)rec[(size_t)hst.stop_at * wrec + 1];
        TopkWork w{{reinterpret_cast<uint64_t*>(b + o_k0), reinterpret_cast<uint64_t*>(b + o_k1)},
                   {reinterpret_cast<int64_t*>(b + o_i0), reinterpret_cast<int64_t*>(b + o_i1)}};
        double* tv = reinterpret_cast<double*>(b + o_tv);
        int64_t* ti = reinterpret_cast<int64_t*>(b + o_ti);
        double* pd = reinterpret_cast<double*>(b + o_pts);
        e = launch_topk(a.score, M, Tk, idx_base, w, tv, ti, s);
        if (e == hipSuccess) e = launch_gather_points(V.Z, ti, idx_base, Tk, d, pd, s);
        if (e == hipSuccess) e = hipMemcpyAsync(gix.data(), ti, sizeof(int64_t) * Tk, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(pts.data(), pd, sizeof(double) * Tk * d, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = stream_wait(s);
        if (e != hipSuccess) break;
        int Tb = 0;
        bool found = false;
        for (; Tb < Tk && gix[Tb] >= 0; ++Tb) found = found || gix[Tb] == gpick;
        if (!found || hst.stop_at < k_from)                   // (a resumed launch must find the pick it stopped at)
            return fail(ABO_EINVAL, "abo_cand_qei_mc: internal error: pick %d is not among the best %d", hst.stop_at + 1, Tb);
        if (int32_t rc = qei_block(g, c, pts.data(), gix.data(), Tb)) return rc;
        qei_mc_view(c, &V);
        e = hipMemsetAsync(&a.st->stop, 0, 2 * sizeof(int32_t), s);
        k_from = hst.stop_at + 1;
    }
    if (e != hipSuccess) return fail(ABO_EHIP, "abo_cand_qei_mc: %s", hipGetErrorString(e));
    for (int j = 0; j < q; ++j) {
        const double* r = &rec[(size_t)j * wrec];
        qei_out[j] = r[0];
        idx_out[j] = (int64_t)r[1];
        for (int i = 0; i < d; ++i) x_out[(size_t)j * d + i] = r[4 + i];
    }
    return ABO_OK;
}

}  // namespace
}  // namespace abo

using namespace abo;

int32_t abo_cand_qei_mc(abo_gp* g, abo_cand* c, int32_t q, double xi, double best_y, const double* base, int32_t S, int32_t base_space,
                        int64_t idx_base, int32_t block, double* x_out, int64_t* idx_out, double* qei_out, abo_qei_stats* stats) {
    const auto t0 = std::chrono::steady_clock::now();
    // every argument check comes before the handles are looked at
    if (!g || !c || !base || !x_out || !idx_out || !qei_out) return fail(ABO_EINVAL, "abo_cand_qei_mc: null argument");
    if (q < 1 || q > QMC_MAXQ) return fail(ABO_EINVAL, "abo_cand_qei_mc: q = %d outside 1..%d", q, QMC_MAXQ);
    if (S < 1 || S > QMC_MAXS) return fail(ABO_EINVAL, "abo_cand_qei_mc: S = %d base samples outside 1..%d", S, QMC_MAXS);
    if (base_space != ABO_HOST && base_space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_cand_qei_mc: unknown memory space %d", base_space);
    if (block != 0 && (block < 16 || block > QEI_MAXT)) return fail(ABO_EINVAL, "abo_cand_qei_mc: block = %d (0 or 16..%d)", block, QEI_MAXT);
    if (idx_base < 0) return fail(ABO_EINVAL, "abo_cand_qei_mc: idx_base = %lld", (long long)idx_base);
    if (!std::isfinite(xi) || !std::isfinite(best_y)) return fail(ABO_EINVAL, "abo_cand_qei_mc: xi and best_y must be finite");
    if (base_space == ABO_HOST)
        for (int64_t i = 0; i < (int64_t)S * q; ++i)
            if (!std::isfinite(base[i])) return fail(ABO_EINVAL, "abo_cand_qei_mc: base[%lld] is not finite", (long long)i);
    const int T = block == 0 ? qei_block_default() : block;
    if (T < 1)
        return fail(ABO_EINVAL, "abo_cand_qei_mc: the process default block size is 0 (the plain loop); the Monte-Carlo q-EI runs only in "
                                "the block form: pass block = 16..%d", QEI_MAXT);
    if (cand_size(c) < q)
        return fail(ABO_EINVAL, "abo_cand_qei_mc: %lld candidates for q = %d distinct picks", (long long)cand_size(c), q);
    QeiBatchStats keep{};
    int32_t rc = qei_mc_open(g, c, q, T, idx_base, &keep);       // (its refusals name abo_cand_qei_mc and their reason)
    if (rc) return rc;
    rc = qei_mc_drive(g, c, q, xi, best_y, base, S, base_space, idx_base, T > QEI_MAXT ? QEI_MAXT : T, x_out, idx_out, qei_out);
    const std::string why = rc ? last_error_text() : std::string();
    QeiMcView V{};
    qei_mc_view(c, &V);
    qei_mc_close(c, keep);
    if (stats) {
        stats->picks = q; stats->block = V.T16; stats->block_builds = V.now.builds;
        stats->block_hits = q - 1 > V.now.builds ? q - 1 - V.now.builds : 0;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        stats->block_ms = V.now.block_ms; stats->pass_ms = V.now.pass_ms; stats->pass_bytes = V.now.pass_bytes; stats->pass_flop = V.now.pass_flop;
    }
    if (rc) return fail(rc, "%s", why.c_str());
    return ABO_OK;
}
