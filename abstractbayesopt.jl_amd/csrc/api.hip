// C-ABI of libabo_hip.so (declared in include/abo_hip.h): handle lifetime and the device-memory pool, the blocked fp64
// factorisation driver (fit / append / remove), NLML / LOO / joint covariance / KG, refinement, the MES entry points that are no
// acquisition pass.  The chunked posterior pass is posterior.hip, scoring and selection acq.hip, resident candidate sets cand.hip,
// their greedy batch selection qei_host.hip; what the five share is declared in abo_state.h — the error slot, the exit flag, the
// pool and the thread-local behind phase_events() are defined here, once.  Host-side orchestration only — all arithmetic is in the
// HIP kernels of gemm.hip / kgen.hip / chol.hip / misc.hip.
//
// Device-resident state of a fitted handle (Np = N rounded up to 128, identity-padded):
//   Xs  [Np][dp]   training points × 1/ell, zero padded (dp = d rounded up to 1,2,4,8,16,32)
//   K   [Np][Np]   K + noise·I, overwritten by its lower Cholesky factor L
//   W   [Np][Np]   L⁻¹ (lower, explicit zeros above)       WT = Wᵀ (upper)
//   alpha, delta [Np]
// Posterior workspace (cached across calls): K_XZ chunk [Mc][Np] candidate-major, partial
// [Np/128][Mc], mu chunk [Mc], full-length mu/var/score arrays, top-k scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <limits>
#include <map>
#include <mutex>
#include <set>
#include <new>
#include <vector>

#include "abo_state.h"
#include "abo_kernels.h"
#include "kgen_core.h"

using namespace abo;

namespace {

thread_local char g_err[512] = "";

}  // namespace

namespace abo {    // shared with test_hooks.hip (abo_state.h)
int32_t fail(int32_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// The end of a call waits for its stream.  hipStreamSynchronize blocks the host thread on an interrupt as soon as the work is not done at
// once: 20 – 40 µs from the last kernel's end to the return, three times a BO step on the incremental path (0.7 ms) and once per 0.15 ms
// step at the reference's own sizes.  Short waits are therefore polled (hipStreamQuery reads the queue's completion signal, ≈ 1 µs a
// call); a wait that outlasts ABO_SPIN_WAIT_US (default 400, 0 = always block) falls back to the blocking call — a 450 ms
// posterior does not spin a core.
hipError_t wait_stream(hipStream_t s) {
    static const long spin_us = [] { const char* e = getenv("ABO_SPIN_WAIT_US"); return e ? atol(e) : 400L; }();
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        bool pending = false;
        for (;;) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) {
                if (pending && e == hipSuccess) (void)hipGetLastError();      // hipErrorNotReady must not stay in the runtime's last-error slot:
                return e;                                                     // the launch wrappers return hipGetLastError()
            }
            pending = true;
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
        }
        (void)hipGetLastError();
    }
    return hipStreamSynchronize(s);
}
}  // namespace abo

namespace {

// ---- process teardown guard (abo_internal.h) -------------------------------------------------------------------------------
std::atomic<bool> g_exiting{false};
std::atomic<bool> g_exit_armed{false};
std::mutex g_exit_mu;
std::vector<void (*)()> g_exit_hooks;
void exit_hook() {
    g_exiting.store(true);
    std::vector<void (*)()> hooks;
    { std::lock_guard<std::mutex> lk(g_exit_mu); hooks.swap(g_exit_hooks); }
    for (auto f : hooks) f();
}
// the library's own unload (dlclose, or static destruction at exit if the atexit hook was never armed)
__attribute__((destructor)) void lib_unload() { g_exiting.store(true); }

// Device-memory pool.  `update` returns a NEW model every BO step (src/surrogates/StandardGP.jl:82)
// and the previous one dies right after, so without a pool every step pays hipMalloc/hipFree for
// ~4 GB of factor + workspace (and the implicit device synchronisations of hipFree).  Freed blocks
// are kept per device (up to ABO_POOL_LIMIT_MB, default 32 GiB) and handed back to the next handle.
struct Pool {
    std::mutex mu;
    std::multimap<size_t, void*> blocks;
    size_t held = 0;
};
Pool g_pool[16];

size_t pool_limit() {
    static size_t lim = [] {
        const char* e = getenv("ABO_POOL_LIMIT_MB");
        return (e ? (size_t)atoll(e) : (size_t)32768) << 20;
    }();
    return lim;
}

size_t round_size(size_t bytes) {
    const size_t g = bytes < ((size_t)1 << 20) ? 4096 : ((size_t)2 << 20);
    return (bytes + g - 1) / g * g;
}

}  // namespace

namespace abo {    // shared with test_hooks.hip (abo_state.h)
hipError_t pool_alloc(int dev, size_t bytes, void** p, size_t* cap) {
    const size_t want = round_size(bytes);
    Pool& pl = g_pool[dev & 15];
    {
        std::lock_guard<std::mutex> lk(pl.mu);
        auto it = pl.blocks.lower_bound(want);
        if (it != pl.blocks.end() && it->first <= want + want / 4 + ((size_t)1 << 20)) {
            *p = it->second; *cap = it->first;
            pl.held -= it->first;
            pl.blocks.erase(it);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) {           // out of memory: give the pool back to the driver and retry once
        std::vector<void*> drop;
        {
            std::lock_guard<std::mutex> lk(pl.mu);
            for (auto& kv : pl.blocks) drop.push_back(kv.second);
            pl.blocks.clear(); pl.held = 0;
        }
        for (void* q : drop) (void)hipFree(q);
        (void)hipGetLastError();
        e = hipMalloc(p, want);
    }
    if (e == hipSuccess) *cap = want;
    return e;
}

void pool_free(int dev, void* p, size_t cap) {
    if (g_exiting.load()) return;        // the process is going away: the driver reclaims device memory, the runtime may be gone
    Pool& pl = g_pool[dev & 15];
    std::vector<void*> evict;
    bool kept = false;
    {
        std::lock_guard<std::mutex> lk(pl.mu);
        // A full pool gives up its LARGEST blocks to keep a smaller one (round 5: after a config-5 model — 17 GB of K_ZX and its
        // factors held — the few-KB buffers of a small model that followed it were hipFree'd and hipMalloc'ed on every BO step,
        // 0.17 → 0.35 ms per step; a large block is the one whose next hipMalloc is amortised over the most work)
        while (pl.held + cap > pool_limit() && !pl.blocks.empty() && std::prev(pl.blocks.end())->first > cap) {
            auto it = std::prev(pl.blocks.end());
            evict.push_back(it->second);
            pl.held -= it->first;
            pl.blocks.erase(it);
        }
        if (pl.held + cap <= pool_limit()) {
            pl.blocks.emplace(cap, p);
            pl.held += cap;
            kept = true;
        }
    }
    for (void* q : evict) (void)hipFree(q);
    if (!kept) (void)hipFree(p);
}
}  // namespace abo

namespace {

void pool_trim(int dev) {
    if (g_exiting.load()) return;
    Pool& pl = g_pool[dev & 15];
    std::vector<void*> drop;
    {
        std::lock_guard<std::mutex> lk(pl.mu);
        for (auto& kv : pl.blocks) drop.push_back(kv.second);
        pl.blocks.clear(); pl.held = 0;
    }
    for (void* q : drop) (void)hipFree(q);
}

std::mutex g_ctx_mu;
std::vector<ExecCtx*> g_ctx_free[16];

// padded coordinate count: 1, 2, 4, 8, 16, 32 (register-resident kernels), beyond that a multiple of 32 (slab kernels)
int dp_for(int d) {
    if (d > 32) return (d + 31) / 32 * 32;
    int p = 1;
    while (p < d) p <<= 1;
    return p;
}

}  // namespace

namespace abo {    // shared with test_hooks.hip (abo_state.h)
std::atomic<uint64_t> g_storage_gen{1};
}  // namespace abo

namespace {
std::atomic<uint64_t> g_append_serial{1};

// contraction engine of the posterior variance: process default (ABO_CONTRACTION = auto | fp64 | int8 | int8:<moduli>),
// overridable per handle (abo_set_contraction)
std::atomic<int> g_oz_engine{-1}, g_oz_nmod{OZ_DEFAULT_NMOD};
}  // namespace

void abo::oz_defaults(int* engine, int* nmod) {
    int e = g_oz_engine.load();
    if (e < 0) {
        e = ABO_CONTRACT_AUTO;
        int n = OZ_DEFAULT_NMOD;
        if (const char* v = getenv("ABO_CONTRACTION")) {
            if (!strncmp(v, "fp64", 4)) e = ABO_CONTRACT_FP64;
            else if (!strncmp(v, "int8", 4)) {
                e = ABO_CONTRACT_INT8;
                if (v[4] == ':') { const int q = atoi(v + 5); if (q >= 8 && q <= OZ_MAXMOD) n = q; }
            }
        }
        g_oz_nmod.store(n);
        g_oz_engine.store(e);
    }
    *engine = e;
    *nmod = g_oz_nmod.load();
}

void abo_gp::free_all() {
#define X(name) name.release();
    ABO_GP_BUFS(X)
#undef X
    oz_N = -1;
    oz_ctr_clean = nullptr;
    if (st && fitted) st->drop_view(N);
    storage_unref(st);
    st = nullptr;
    if (ctx) {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        g_ctx_free[prm.device & 15].push_back(ctx);
        ctx = nullptr; stream = nullptr;
    }
}

KgenArgs abo::kgen_model_args(const abo_gp* g, bool with_mean) {
    KgenArgs ka{};
    ka.Xs = g->st->Xs.as<double>(); ka.N = (int)g->npts; ka.Np = (int)g->Np; ka.d = g->d; ka.dp = g->dp;
    ka.family = g->prm.family; ka.s = 1.0 / g->prm.ell; ka.sigma_f2 = g->prm.sigma_f2; ka.pt = g->p_out;
    if (with_mean) {
        ka.mean_c = g->prm.mean_c;
        for (int q = 0; q < MAX_P; ++q) ka.mean_vec[q] = g->mean_vec[q];
    }
    return ka;
}

namespace abo {    // shared with the other host units (abo_state.h)

int32_t copy_in(void* dst, const void* src, size_t bytes, int32_t space, hipStream_t s) {
    if (bytes == 0) return ABO_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, space == ABO_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    return ABO_OK;
}

int32_t copy_out(void* dst, const void* src, size_t bytes, int32_t space, hipStream_t s) {
    if (bytes == 0) return ABO_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, space == ABO_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return ABO_OK;
}

float ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }   // (an event that was never recorded)
    return ms;
}

// Phase events.  Every call is bracketed by two events (its total); the events INSIDE a call — fit phases, per-chunk kernel
// brackets of the posterior — are profiling instrumentation: each costs a host call and a marker packet between two kernels,
// ≈ 40 of them per BO step, which at the reference's own sizes (a step of 0.2 ms) is a fifth of the step.  ABO_PHASE_EVENTS=0
// leaves them out (the phase fields of abo_timings then read 0, the totals stay); default on.
// ABO_PHASE_EVENTS: 1 = always, 0 = never, unset = automatic — on, except while the calling thread works on a model of one row block
// (N ≤ 128: the reference's own loops, where the step is 0.2 ms and the instrumentation a fifth of it).
// The thread-local is written in this unit alone (check_fitted, fit_impl, append_impl) and read through phase_events(), which the
// other units call: ONE definition of both.
namespace { thread_local int64_t tl_phase_np = (int64_t)1 << 40; }    // padded factor rows of the handle the current call works on
bool phase_events() {
    static const int mode = [] { const char* e = getenv("ABO_PHASE_EVENTS"); return !e ? -1 : (e[0] == '0' ? 0 : 1); }();
    return mode < 0 ? tl_phase_np > TB : mode == 1;
}

}  // namespace abo

namespace {

int32_t factorise(abo_gp* g, double noise, int64_t* info_host);
int32_t fit_small(abo_gp* g, double noise, int64_t* info_host);

// the scalars and phase timings of a finished fit (h_sc / h_info have landed: the stream has been synchronised since)
void fit_collect(abo_gp* g) {
    g->logdet = g->h_sc()[0];
    g->quad = g->h_sc()[1];
    g->tm.fit_total_ms = ev_ms(g->evs()[EV_FIT_BEGIN], g->evs()[EV_FIT_END]);
    if (!phase_events()) {
        g->tm.fit_kernel_matrix_ms = g->tm.fit_cholesky_ms = g->tm.fit_inverse_ms = g->tm.fit_alpha_ms = 0.0;
        return;
    }
    if (g->fit_small_path) {
        g->tm.fit_kernel_matrix_ms = 0.0;
        g->tm.fit_cholesky_ms = ev_ms(g->evs()[EV_FIT_KMAT], g->evs()[EV_FIT_CHOL]);      // the one launch
        g->tm.fit_inverse_ms = 0.0;
        g->tm.fit_alpha_ms = 0.0;
    } else {
        g->tm.fit_kernel_matrix_ms = ev_ms(g->evs()[EV_FIT_BEGIN], g->evs()[EV_FIT_KMAT]);
        g->tm.fit_cholesky_ms = ev_ms(g->evs()[EV_FIT_KMAT], g->evs()[EV_FIT_CHOL]);
        g->tm.fit_inverse_ms = ev_ms(g->evs()[EV_FIT_CHOL], g->evs()[EV_FIT_INV]);
        g->tm.fit_alpha_ms = ev_ms(g->evs()[EV_FIT_INV], g->evs()[EV_FIT_END]);
    }
    g->tm.fit_total_ms = ev_ms(g->evs()[EV_FIT_BEGIN], g->evs()[EV_FIT_END]);
}

}  // namespace

namespace abo {    // shared with test_hooks.hip (abo_state.h)

// Right-looking blocked Cholesky of K [Np][ld], 128-wide panels; the 128×128 inverses of the diagonal blocks go to W / WT.
int32_t chol_blocked(double* K, double* W, double* WT, double* T, int64_t ld, int Np, int64_t* info, const CholBlocking& blk, hipStream_t s) {
    const bool split = Np > TB;                            // a single block has no chain: factor + inverse in one launch
    // Two-level blocking: inside a strip of SW columns the 128-wide panels update only the rest of the strip
    // (K = 128 products on a tall, narrow block); the matrix behind the strip is updated once per strip with
    // K = SW — a quarter of the read-modify-write passes over the trailing matrix and four times longer k loops
    // per tile than a panel-by-panel SYRK.
    const int SW = blk.SW;
    // Third level: strips grouped into super-strips of 1024 columns — behind a strip only the rest of its super-strip is updated
    // (K = SW), the matrix behind the super-strip once per super-strip with K = SS: half the passes over the trailing matrix and
    // tiles twice as long (Cholesky at N = 16384 35.0 → 32.8 ms, at N = 8192 8.20 → 8.23: profiles/r03_chol_super_sweep.txt).  A
    // super-strip pays while the square update behind it is large — its in-super-strip update is a launch of 4 × T tiles that lasts
    // ≈ 150 µs whatever T is, against K = 1024 tiles at 70 TFLOP/s instead of 52 (profiles/r04_fit_trace_summary.txt) — so
    // super-strips are used while at least 6144 rows remain, plain strips from there on.
    const int SSmax = blk.SSmax, super_rows = blk.super_rows;
    // Panel chain: potf2 of the diagonal block (potf2_pipe_kernel) → triangular solve of the rows below it from the operand stream that
    // kernel leaves (trsm_stream_kernel; the stream lives in T, which the factorisation does not use — the blocked inverse behind it
    // does) → in-strip update.  The 128×128 inverses of the diagonal blocks (the seeds of the blocked L⁻¹ below) are not on that chain:
    // all of them are formed by ONE batched launch behind the factorisation.  Measured and not adopted (profiles/r05_notes.md D, removed
    // from the library in round 6): a two-stream look-ahead, one launch per panel with in-launch hand-overs, 256 × 128 trailing tiles;
    // round 6: the same look-ahead on CU-MASKED streams (hipExtStreamCreateWithCUMask: chain and trailing update on disjoint compute
    // units, so the chain never waits for a slot) — 7.4 – 9.1 ms against 7.0 at N = 8192 (profiles/r06_chol_lookahead_cumask_ab.txt).
    double* trsm_ops = T;
    for (int S0 = 0, SS = SW; S0 < Np; S0 += SS) {
        SS = (Np - S0) >= super_rows ? SSmax : SW;
        const int ss = (Np - S0) < SS ? (Np - S0) : SS;
        for (int s0 = S0; s0 < S0 + ss; s0 += SW) {
            const int sw = (S0 + ss - s0) < SW ? (S0 + ss - s0) : SW;
            for (int r0 = s0; r0 < s0 + sw; r0 += TB) {
                const int rem = Np - r0 - TB;
                if (!split) { HIPCHK(launch_chol_diag(K, W, WT, ld, r0, info, s)); break; }
                HIPCHK(launch_potf2_diag(K, W, WT, ld, r0, info, s, trsm_ops, true));
                if (rem <= 0) break;
                HIPCHK(launch_trsm_stream(K, trsm_ops, ld, r0, rem, info, s));
                // in-strip update  A[r,c] −= L[r,p]·L[c,p]ᵀ  for the strip's remaining columns c, lower tiles only
                const int ncol = s0 + sw - r0 - TB;
                if (ncol > 0) {
                    GemmArgs u{};
                    u.A = K + (int64_t)(r0 + TB) * ld + r0; u.lda = ld;
                    u.B = u.A; u.ldb = ld;
                    u.C = K + (int64_t)(r0 + TB) * ld + (r0 + TB); u.ldc = ld;
                    u.M = rem; u.N = ncol; u.K = TB; u.kmode = K_FULL; u.lower_only = 1; u.batch = 1;
                    u.alpha = -1.0; u.beta = 1.0; u.info = info;
                    HIPCHK(launch_gemm_nt(u, s));
                }
            }
            // update behind the strip, inside its super-strip:  A[r,c] −= L[r,strip]·L[c,strip]ᵀ  for all rows r below the strip and
            // the super-strip's remaining columns c (lower tiles only), K = sw
            const int rows = Np - s0 - sw;
            const int cols = S0 + ss - s0 - sw;
            if (rows > 0 && cols > 0) {
                GemmArgs u{};
                u.A = K + (int64_t)(s0 + sw) * ld + s0; u.lda = ld;
                u.B = u.A; u.ldb = ld;
                u.C = K + (int64_t)(s0 + sw) * ld + (s0 + sw); u.ldc = ld;
                u.M = rows; u.N = cols; u.K = sw; u.kmode = K_FULL; u.lower_only = 1; u.batch = 1;
                u.alpha = -1.0; u.beta = 1.0; u.info = info;
                HIPCHK(launch_gemm_nt(u, s));
            }
        }
        const int rest = Np - S0 - ss;
        if (rest > 0) {
            // trailing update behind the super-strip  A[r,c] −= L[r,super]·L[c,super]ᵀ  on the lower triangle, K = ss
            GemmArgs u{};
            u.A = K + (int64_t)(S0 + ss) * ld + S0; u.lda = ld;
            u.B = u.A; u.ldb = ld;
            u.C = K + (int64_t)(S0 + ss) * ld + (S0 + ss); u.ldc = ld;
            u.M = rest; u.N = rest; u.K = ss; u.kmode = K_FULL; u.lower_only = 1; u.batch = 1;
            u.alpha = -1.0; u.beta = 1.0; u.info = info;
            HIPCHK(launch_gemm_nt(u, s));
        }
    }
    if (split) HIPCHK(launch_trtri_diag_batched(K, W, WT, ld, Np / TB, info, s));
    return ABO_OK;
}

// L⁻¹ by recursive doubling from the diagonal blocks' inverses.
int32_t trinv_blocked(double* K, double* W, double* WT, double* T, int64_t ld, int Np, int64_t* info, hipStream_t s) {
    // W = L⁻¹: [[W11,0],[−W22·L21·W11, W22]] level by level (block size s doubles each level)
    double* Tt = T;
    for (int64_t sz = TB; sz < Np; sz *= 2) {
        const int64_t two = 2 * sz;
        const int nfull = (int)(Np / two);
        const int64_t rrem = Np - (int64_t)nfull * two;
        for (int pass = 0; pass < 2; ++pass) {
            const bool ragged = pass == 1;
            if (ragged && rrem <= sz) break;
            if (!ragged && nfull == 0) continue;
            const int64_t r1 = ragged ? (int64_t)nfull * two : 0;
            const int64_t r2 = r1 + sz;
            const int64_t s2 = ragged ? rrem - sz : sz;
            const int batch = ragged ? 1 : nfull;
            const int64_t bstride = two * (ld + 1);
            double* Tp = Tt + (ragged ? (int64_t)nfull * sz * sz : 0);
            GemmArgs a{};   // Tt[j][i] = Σ_k WT11[j][k]·L21[i][k]
            a.A = WT + r1 * ld + r1; a.lda = ld; a.sA = bstride;
            a.B = K + r2 * ld + r1; a.ldb = ld; a.sB = bstride;
            a.C = Tp; a.ldc = sz; a.sC = sz * sz;
            a.M = (int)sz; a.N = (int)s2; a.K = (int)sz; a.kmode = K_A_UPPER; a.batch = batch;
            a.alpha = 1.0; a.beta = 0.0; a.info = info;
            HIPCHK(launch_gemm_nt(a, s));
            GemmArgs b{};   // W21[i][j] = −Σ_k W22[i][k]·Tt[j][k]   (+ transposed copy into WT)
            b.A = W + r2 * ld + r2; b.lda = ld; b.sA = bstride;
            b.B = Tp; b.ldb = sz; b.sB = sz * sz;
            b.C = W + r2 * ld + r1; b.ldc = ld; b.sC = bstride;
            b.Ct = WT + r1 * ld + r2; b.ldct = ld; b.sCt = bstride;
            b.M = (int)s2; b.N = (int)sz; b.K = (int)s2; b.kmode = K_A_LOWER; b.batch = batch;
            b.alpha = -1.0; b.beta = 0.0; b.info = info;
            HIPCHK(launch_gemm_nt(b, s));
        }
    }
    return ABO_OK;
}

}  // namespace abo

namespace {

// Right-looking blocked Cholesky, 128-wide panels, then L⁻¹ by recursive doubling.
// info_host == nullptr: launches only — the caller synchronises later and then looks at g->h_info / calls fit_collect().
int32_t factorise(abo_gp* g, double noise, int64_t* info_host) {
    hipStream_t s = g->stream;
    Storage* st = g->st;
    const int Np = (int)g->Np, N = (int)g->N;
    const int64_t ld = st->cap;
    double* K = st->K.as<double>();
    double* W = st->W.as<double>();
    double* WT = st->WT.as<double>();
    HIPCHK(g->info.ensure(sizeof(int64_t)));
    int64_t* info = g->info.as<int64_t>();              // the LAPACK-style status

    HIPCHK(hipEventRecord(g->evs()[EV_FIT_BEGIN], s));
    // whole capacity region: zeros, identity on the padded diagonal (rows ≥ N), K on the active part.  With a panel chain (more than
    // one block) rows < Np of W / WT are zeroed by the chain's own launches — the idle workgroups of each diagonal-block launch take
    // that panel's rows (chol.hip: potf2_pipe_kernel) — instead of two whole-matrix memsets in front of the fit (148 µs at N = 8192).
    const bool split = Np > TB;                            // a single block has no chain: factor + inverse in one launch
    if (ld > Np) HIPCHK(hipMemsetAsync(K, 0, sizeof(double) * ld * ld, s));
    if (!split) {
        HIPCHK(hipMemsetAsync(W, 0, sizeof(double) * ld * ld, s));
        HIPCHK(hipMemsetAsync(WT, 0, sizeof(double) * ld * ld, s));
    } else if (ld > Np) {
        HIPCHK(hipMemsetAsync(W + (int64_t)Np * ld, 0, sizeof(double) * (ld - Np) * ld, s));
        HIPCHK(hipMemsetAsync(WT + (int64_t)Np * ld, 0, sizeof(double) * (ld - Np) * ld, s));
    }
    KgenArgs ka = kgen_model_args(g, false);
    ka.Z = st->Xraw.as<double>(); ka.Kout = K; ka.ldk = ld; ka.M = g->npts; ka.Mc = Np;
    ka.pc = g->p_out; ka.point_major = 1;                        // K_XX: rows and columns point-major → symmetric
    HIPCHK(launch_kgen(ka, s));
    HIPCHK(launch_diag_fix(K, ld, N, (int)ld, noise, s, info));      // also resets the status word
    if (ld > Np) {
        HIPCHK(launch_set_diag(W, ld, Np, (int)ld, 1.0, s));
        HIPCHK(launch_set_diag(WT, ld, Np, (int)ld, 1.0, s));
    }
    PHASE_EVENT(g->evs()[EV_FIT_KMAT], s);

    // (the operand stream of the panel solve lives in T, which the factorisation does not use — the blocked inverse behind it does)
    if (split) HIPCHK(g->T.ensure(TRSM_STREAM_BYTES));
    { const int32_t rc = chol_blocked(K, W, WT, g->T.as<double>(), ld, Np, info, CholBlocking{}, s); if (rc) return rc; }
    PHASE_EVENT(g->evs()[EV_FIT_CHOL], s);
    // no host round trip here: after a failed pivot every later kernel of the fit either exits on `info` (the GEMMs) or
    // works on finite leftovers whose results are discarded; `info` is read once, with the scalars, at the end

    { const int32_t rc = trinv_blocked(K, W, WT, g->T.as<double>(), ld, Np, info, s); if (rc) return rc; }
    PHASE_EVENT(g->evs()[EV_FIT_INV], s);
    // alpha = Wᵀ(W·delta)
    HIPCHK(launch_trmv(W, ld, st->delta.as<double>(), g->tvec.as<double>(), Np, 1, s));
    HIPCHK(launch_trmv(WT, ld, g->tvec.as<double>(), g->alpha.as<double>(), Np, 0, s));
    HIPCHK(launch_nlml_terms(K, ld, st->delta.as<double>(), g->alpha.as<double>(), N, g->scal.as<double>(), s));
    HIPCHK(hipEventRecord(g->evs()[EV_FIT_END], s));
    g->fit_small_path = false;
    HIPCHK(hipMemcpyAsync(g->h_sc(), g->scal.as<double>(), 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&g->h_info(), info, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (!info_host) return ABO_OK;        // deferred: fit_collect() after the caller's synchronisation
    HIPCHK(wait_stream(s));
    *info_host = g->h_info();
    if (g->h_info() == 0) fit_collect(g);   // else the caller decides (retry with jitter or ENOTPD)
    return ABO_OK;
}

// The whole fit of a small model (N ≤ 128, d ≤ 16, capacity 128) in one launch; same outputs and timing slots as factorise().
int32_t fit_small(abo_gp* g, double noise, int64_t* info_host) {
    hipStream_t s = g->stream;
    Storage* st = g->st;
    int64_t* info = g->info.as<int64_t>();
    HIPCHK(hipEventRecord(g->evs()[EV_FIT_BEGIN], s));
    PHASE_EVENT(g->evs()[EV_FIT_KMAT], s);                            // (the launch resets the status word itself)
    FitSmallArgs fs{};
    fs.Xraw = st->Xraw.as<double>(); fs.y = st->ybuf.as<double>(); fs.Xs = st->Xs.as<double>(); fs.delta = st->delta.as<double>();
    if (g->in_x) { fs.Xraw = g->in_x; fs.y = g->in_y; fs.Xkeep = st->Xraw.as<double>(); fs.ykeep = st->ybuf.as<double>(); }
    fs.alpha = g->alpha.as<double>(); fs.scal = g->scal.as<double>();
    fs.N = (int)g->N; fs.d = g->d; fs.dp = g->dp; fs.family = g->prm.family;
    fs.s = 1.0 / g->prm.ell; fs.sigma_f2 = g->prm.sigma_f2; fs.noise = noise; fs.mean_c = g->prm.mean_c;
    HIPCHK(launch_fit_small(st->K.as<double>(), st->W.as<double>(), st->WT.as<double>(), info, fs, s));
    PHASE_EVENT(g->evs()[EV_FIT_CHOL], s);
    HIPCHK(hipEventRecord(g->evs()[EV_FIT_END], s));
    g->fit_small_path = true;
    HIPCHK(hipMemcpyAsync(g->h_sc(), g->scal.as<double>(), 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&g->h_info(), info, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (!info_host) return ABO_OK;        // deferred: fit_collect() after the caller's synchronisation
    HIPCHK(wait_stream(s));
    *info_host = g->h_info();
    if (g->h_info() == 0) fit_collect(g);
    return ABO_OK;
}

}  // namespace

namespace abo {    // shared with test_hooks.hip (abo_state.h)
int32_t check_fitted(abo_gp* g, int32_t d) {
    if (!g) return fail(ABO_EINVAL, "null handle");
    tl_phase_np = g->Np;                             // (every posterior / acquisition entry point passes here first)
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    if (d != g->d) return fail(ABO_EDIM, "DimensionMismatch: candidate dimension %d, model dimension %d", d, g->d);
    return ABO_OK;
}

int32_t stage_candidates(abo_gp* g, const double* Z, int64_t M, int32_t z_space, const double** Zd) {
    if (z_space == ABO_DEVICE) { *Zd = Z; return ABO_OK; }
    HIPCHK(g->Zdev.ensure(sizeof(double) * M * g->d));
    HIPCHK(hipMemcpyAsync(g->Zdev.p, Z, sizeof(double) * M * g->d, hipMemcpyHostToDevice, g->stream));
    *Zd = g->Zdev.as<double>();
    return ABO_OK;
}
}  // namespace abo

namespace {

// Full refit into a fresh Storage of capacity max(N, n_max) points.  X/y: caller buffers (host or device).
// Gradient-enhanced models (p_out > 1): y holds p_out values per point, by outputs at the ABI (y[q·N + i]) or — internal
// callers, y_point_major — already in the factor's point-major order (y[i·p + q]).
// defer: queue the fit's launches and return without waiting (no jitter retries then): the handle is provisionally marked
// fitted so that posterior launches can be queued behind it; the caller synchronises and calls fit_finish().
int32_t fit_impl(abo_gp* g, const double* X, int64_t N, int d, const double* y, int32_t space, int64_t* info,
                 int y_point_major = 0, bool defer = false) {
    hipStream_t s = g->stream;
    g->from_append = false;
    g->ap_x.clear();
    Storage* st = new (std::nothrow) Storage();
    if (!st) return fail(ABO_ENOMEM, "abo_fit: host allocation failed");
    st->set_device(g->prm.device);
    st->d = d; st->dp = dp_for(d);
    const int P = g->p_out;                              // N below = number of training POINTS
    const int64_t R = (int64_t)P * N;                    // factor rows
    const int64_t want = (int64_t)P * (g->prm.n_max > N ? g->prm.n_max : N);
    st->cap = pad_up(want, TB);
    const int64_t cap = st->cap;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = st->Xraw.ensure(sizeof(double) * cap * d);
    if (e == hipSuccess) e = st->Xs.ensure(sizeof(double) * cap * st->dp);
    if (e == hipSuccess) e = st->ybuf.ensure(sizeof(double) * cap);
    if (e == hipSuccess) e = st->delta.ensure(sizeof(double) * cap);
    if (e == hipSuccess) e = st->K.ensure(sizeof(double) * cap * cap);
    if (e == hipSuccess) e = st->W.ensure(sizeof(double) * cap * cap);
    if (e == hipSuccess) e = st->WT.ensure(sizeof(double) * cap * cap);
    if (e != hipSuccess) {
        storage_unref(st);
        return fail(e == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "abo_fit: device allocation failed: %s", hipGetErrorString(e));
    }
    const int64_t Np = pad_up(R, TB);
    {
        hipError_t eh = g->alpha.ensure(sizeof(double) * cap);      // the handle's own buffers, BEFORE the previous storage goes back to
        if (eh == hipSuccess) eh = g->tvec.ensure(sizeof(double) * cap);      // the pool: nothing handed out below may be memory the
        if (eh == hipSuccess) eh = g->T.ensure(sizeof(double) * Np * Np);     // caller's X / y still live in (refit after append)
        if (eh == hipSuccess) eh = g->info.ensure(sizeof(int64_t));
        if (eh == hipSuccess) eh = g->scal.ensure(sizeof(double) * 8);
        if (eh != hipSuccess) {
            storage_unref(st);
            return fail(eh == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "abo_fit: device allocation failed: %s", hipGetErrorString(eh));
        }
    }
    // N ≤ 128, d ≤ 16, no spare capacity: the whole fit is one launch (chol.hip, mode 3 of the diagonal-block kernel)
    const bool fused_small = P == 1 && cap == TB && st->dp <= 16;
    // Inputs.  Device arrays of a StandardGP are read by the fit's first launch itself, which also writes the model's own copies — the
    // prep launch (larger models; issued right here), or the one-launch fit of a fresh handle — instead of two staging copies and three
    // tiny launches in front of the kernel matrix.  Everything else is staged as before.  All of it BEFORE the previous storage is
    // dropped: X / y may alias it (refit after append).
    g->in_x = g->in_y = nullptr;
    const bool direct = P == 1 && space == ABO_DEVICE && N > 0;
    int32_t rc = ABO_OK;
    if (direct && fused_small && g->st == nullptr) {        // (a handle that holds a storage stages: its launch runs behind the drop)
        g->in_x = X; g->in_y = y;
    } else if (!direct || fused_small) {
        rc = copy_in(st->Xraw.p, X, sizeof(double) * N * d, space, s);
        // (gradient-enhanced: staged in K — overwritten by the kernel matrix later — and reordered into ybuf below)
        if (!rc) rc = copy_in(P == 1 ? st->ybuf.p : st->K.p, y, sizeof(double) * R, space, s);
        if (rc) { storage_unref(st); return rc; }
    }
    if (P == 1 && !fused_small)
        HIPCHK(launch_fit_prep(direct ? X : st->Xraw.as<double>(), direct ? y : st->ybuf.as<double>(), st->Xraw.as<double>(),
                               st->ybuf.as<double>(), st->Xs.as<double>(), st->delta.as<double>(), g->alpha.as<double>(), (int)N, (int)cap,
                               d, st->dp, 1.0 / g->prm.ell, g->prm.mean_c, s));
    if (g->st) HIPCHK(wait_stream(s));         // a fresh handle (what update() makes) has nothing the inputs could alias
    if (g->st && g->fitted) g->st->drop_view(g->N);
    g->fitted = false;
    storage_unref(g->st);
    g->st = st;
    g->npts = N; g->N = R; g->d = d; g->dp = st->dp; g->Np = Np;
    tl_phase_np = Np;
    if (defer) {
        rc = fused_small ? fit_small(g, g->prm.noise_var, nullptr) : factorise(g, g->prm.noise_var, nullptr);
        if (rc) return rc;
        st->noise_used = g->prm.noise_var;
        st->add_view(R);
        g->fitted = true;                 // provisional until fit_finish()
        return ABO_OK;
    }
    if (fused_small) {
        int64_t inf = 0;
        double noise = g->prm.noise_var;
        for (int attempt = 0;; ++attempt) {
            rc = fit_small(g, noise, &inf);
            if (rc) return rc;
            if (inf == 0) break;
            if (!(g->prm.jitter > 0.0) || attempt >= 4) {
                if (info) *info = inf;
                return fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld",
                            (long long)inf);
            }
            noise = g->prm.noise_var + g->prm.jitter * std::pow(10.0, attempt);
        }
        st->noise_used = noise;
        st->add_view(R);
        g->fitted = true;
        return ABO_OK;
    }
    if (P > 1) {                                         // point-major rows i·p + q, output q centred by mean_vec[q]
        HIPCHK(launch_scale_points(st->Xraw.as<double>(), st->Xs.as<double>(), (int)N, (int)cap, d, st->dp, 1.0 / g->prm.ell, s));
        MeanVec mv{};
        for (int q = 0; q < P; ++q) mv.c[q] = g->mean_vec[q];
        HIPCHK(launch_center_grad(st->K.as<double>(), st->ybuf.as<double>(), st->delta.as<double>(), (int)N, P, (int)cap, mv,
                                  y_point_major, s));
        HIPCHK(hipMemsetAsync(g->alpha.p, 0, sizeof(double) * cap, s));
    }

    int64_t inf = 0;
    double noise = g->prm.noise_var;
    for (int attempt = 0;; ++attempt) {
        rc = factorise(g, noise, &inf);
        if (rc) return rc;
        if (inf == 0) break;
        if (!(g->prm.jitter > 0.0) || attempt >= 4) {
            if (info) *info = inf;
            return fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld",
                        (long long)inf);
        }
        noise = g->prm.noise_var + g->prm.jitter * std::pow(10.0, attempt);
    }
    st->noise_used = noise;
    st->add_view(R);
    g->fitted = true;
    return ABO_OK;
}

// Bordered ("rank-1 append") update: view `g` (N points) → new view `n` (N+1 points) sharing g's storage.
//   k = k(X, x*),  l = W·k,  l_nn² = k** + noise − ‖l‖²,  v = Wᵀ·l = K⁻¹k
//   L[N] = [lᵀ, l_nn]      W[N] = [−vᵀ/l_nn, 1/l_nn]      β = (δ* − kᵀα)/l_nn²      α' = [α − βv ; β]
// Falls back to a full refit (new storage, doubled capacity) when the capacity is used up or when
// another view already appended to the shared storage (copy-on-write for diverging histories).
int32_t append_impl(abo_gp* g, abo_gp* n, const double* x, double y, int64_t* info) {
    Storage* st = g->st;
    const int d = g->d;
    const int64_t N = g->N;
    hipStream_t s = n->stream;
    if (N + 1 > st->cap || !st->claim_rows(N, N + 1)) {
        // gather this view's data on the device and refit with room to grow
        ScratchBuf xs(g->prm.device, s), ys(g->prm.device, s);
        DevBuf& xb = xs.b;
        DevBuf& yb = ys.b;
        HIPCHK(xb.ensure(sizeof(double) * (N + 1) * d));
        HIPCHK(yb.ensure(sizeof(double) * (N + 1)));
        HIPCHK(hipMemcpyAsync(xb.p, st->Xraw.p, sizeof(double) * N * d, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(yb.p, st->ybuf.p, sizeof(double) * N, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(xb.as<double>() + N * d, x, sizeof(double) * d, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(yb.as<double>() + N, &y, sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(wait_stream(s));
        if (n->prm.n_max < 2 * (N + 1)) n->prm.n_max = 2 * (N + 1);
        return fit_impl(n, xb.as<double>(), N + 1, d, yb.as<double>(), ABO_DEVICE, info);
    }
    // rows [N, N + 1) are claimed: every failure below gives them back
    struct Claim { Storage* st; int64_t n; bool keep = false; ~Claim() { if (!keep) st->drop_view(n); } } claim{st, N + 1};
    const int64_t ld = st->cap;
    const int64_t Np = g->Np;                       // padded size of the OLD view
    const int64_t Np1 = pad_up(N + 1, TB);
    HIPCHK(n->alpha.ensure(sizeof(double) * ld));
    HIPCHK(n->vext.ensure(sizeof(double) * ld));
    HIPCHK(n->tvec.ensure(sizeof(double) * ld * 2));
    HIPCHK(n->Kxz.ensure(sizeof(double) * 16 * Np));
    HIPCHK(n->info.ensure(sizeof(int64_t)));
    HIPCHK(n->scal.ensure(sizeof(double) * 8));
    double* Xraw = st->Xraw.as<double>();
    // new point: raw coordinates, scaled coordinates, centred target (rows N — beyond every older view)
    if (d <= APPEND_POINT_MAXD && st->dp <= APPEND_POINT_MAXD) {
        HIPCHK(launch_append_point(x, d, st->dp, 1.0 / g->prm.ell, y, g->prm.mean_c, Xraw + N * d, st->Xs.as<double>() + N * st->dp,
                                   st->ybuf.as<double>() + N, st->delta.as<double>() + N, n->info.as<int64_t>(), s));
    } else {
        HIPCHK(hipMemcpyAsync(Xraw + N * d, x, sizeof(double) * d, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(st->ybuf.as<double>() + N, &y, sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(launch_scale_points(Xraw + N * d, st->Xs.as<double>() + N * st->dp, 1, 1, d, st->dp, 1.0 / g->prm.ell, s));
        HIPCHK(launch_center(st->ybuf.as<double>() + N, st->delta.as<double>() + N, 1, 1, g->prm.mean_c, s));
        HIPCHK(hipMemsetAsync(n->info.p, 0, sizeof(int64_t), s));
    }
    // k = k(X, x*): one kernel evaluation per training point (the training points play the candidates of the
    // column kernel; same scaled differences and the same kappa as kgen, so the values are bit-identical to a refit's)
    HIPCHK(launch_cand_newcol(st->Xs.as<double>() + N * st->dp, Xraw, n->Kxz.as<double>(), 1, N, 0, d, st->dp, g->prm.family,
                              1.0 / g->prm.ell, g->prm.sigma_f2, s));
    double* krow = n->Kxz.as<double>();
    double* lvec = n->tvec.as<double>();
    double* vvec = n->tvec.as<double>() + ld;
    // only rows/columns < N: anything beyond may be the stale remains of a discarded branch
    tl_phase_np = Np1;
    const bool timed = phase_events();
    // (scratch slots EV_BASE + 0 … 1: begin and end of the two mat-vecs — an append runs no posterior pass)
    if (timed) { HIPCHK(n->events(EV_BASE + 2)); HIPCHK(hipEventRecord(n->evs()[EV_BASE], s)); }
    HIPCHK(launch_trmv(st->W.as<double>(), ld, krow, lvec, (int)N, 1, s));
    HIPCHK(launch_trmv(st->WT.as<double>(), ld, lvec, vvec, (int)N, 0, s));
    if (timed) HIPCHK(hipEventRecord(n->evs()[EV_BASE + 1], s));
    AppendArgs aa{};
    aa.L = st->K.as<double>(); aa.W = st->W.as<double>(); aa.WT = st->WT.as<double>(); aa.ld = ld;
    aa.krow = krow; aa.lvec = lvec; aa.vvec = vvec; aa.alpha_old = g->alpha.as<double>(); aa.alpha_new = n->alpha.as<double>();
    aa.vext = n->vext.as<double>(); aa.delta = st->delta.as<double>(); aa.N = (int)N; aa.cap = (int)ld;
    aa.kss = g->prm.sigma_f2 + st->noise_used; aa.scal = n->scal.as<double>(); aa.info = n->info.as<int64_t>();
    HIPCHK(launch_append(aa, s));
    double sc[4];
    int64_t inf = 0;
    PinStage pin(n->ctx);                            // the NEW handle's staging block: `g` may be in use by another thread (a copy of it)
    HIPCHK(pin.d2h(sc, n->scal.p, sizeof sc, s));
    HIPCHK(pin.d2h(&inf, n->info.p, sizeof inf, s));
    HIPCHK(wait_stream(s));
    pin.flush();
    if (inf != 0) {
        if (info) *info = inf;
        return fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld",
                    (long long)inf);
    }
    storage_unref(n->st);
    st->refs.fetch_add(1);
    n->st = st;
    claim.keep = true;                               // (registered by claim_rows)
    n->N = N + 1; n->npts = N + 1; n->Np = Np1; n->d = d; n->dp = st->dp;
    n->from_append = true;
    // the two triangular mat-vecs l = L⁻¹k, v = L⁻ᵀl: each streams one triangle of its matrix once (8·N²/2 bytes)
    n->tm.append_trmv_ms = timed ? ev_ms(n->evs()[EV_BASE], n->evs()[EV_BASE + 1]) : 0.0;
    n->tm.append_trmv_bytes = 8.0 * (double)N * (double)N;
    n->ap_s2 = sc[0]; n->ap_beta = sc[1];
    n->ap_serial = g_append_serial.fetch_add(1);
    n->ap_x.assign(x, x + d);
    n->logdet = g->logdet + 2.0 * std::log(sc[2]);
    n->quad = g->quad + sc[1] * sc[1] * sc[0];
    n->fitted = true;
    return ABO_OK;
}

// Gradient-enhanced model: one more observation (f and its gradient at x) = p_out more rows at the END of the point-major
// factor, appended one row at a time with the bordered update above; row (N, q) sees the rows (N, q' < q) appended just
// before it.  The kernel row comes from the multi-output generator (analytic derivative blocks), everything else is the
// single-row machinery.  yv: p_out host values {f, ∂f/∂x_1 …}.
int32_t append_grad_impl(abo_gp* g, abo_gp* n, const double* x, const double* yv, int64_t* info) {
    Storage* st = g->st;
    const int d = g->d, P = g->p_out;
    const int64_t R = g->N, npts = g->npts;
    hipStream_t s = n->stream;
    if (R + P > st->cap || !st->claim_rows(R, R + P)) {
        ScratchBuf xs(g->prm.device, s), ys(g->prm.device, s);
        DevBuf& xb = xs.b;
        DevBuf& yb = ys.b;
        HIPCHK(xb.ensure(sizeof(double) * (npts + 1) * d));
        HIPCHK(yb.ensure(sizeof(double) * (R + P)));
        HIPCHK(hipMemcpyAsync(xb.p, st->Xraw.p, sizeof(double) * npts * d, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(yb.p, st->ybuf.p, sizeof(double) * R, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(xb.as<double>() + npts * d, x, sizeof(double) * d, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(yb.as<double>() + R, yv, sizeof(double) * P, hipMemcpyHostToDevice, s));
        HIPCHK(wait_stream(s));
        if (n->prm.n_max < 2 * (npts + 1)) n->prm.n_max = 2 * (npts + 1);
        return fit_impl(n, xb.as<double>(), npts + 1, d, yb.as<double>(), ABO_DEVICE, info, /*y_point_major=*/1);
    }
    struct Claim { Storage* st; int64_t n; bool keep = false; ~Claim() { if (!keep) st->drop_view(n); } } claim{st, R + P};
    const int64_t ld = st->cap;
    HIPCHK(n->alpha.ensure(sizeof(double) * ld));
    HIPCHK(n->T.ensure(sizeof(double) * ld));              // second alpha buffer (the rows alternate between the two)
    HIPCHK(n->vext.ensure(sizeof(double) * ld * P));
    HIPCHK(n->tvec.ensure(sizeof(double) * ld * 2));
    HIPCHK(n->Kxz.ensure(sizeof(double) * 16 * ld));
    HIPCHK(n->info.ensure(sizeof(int64_t)));
    HIPCHK(n->scal.ensure(sizeof(double) * 4 * MAX_P));
    double* Xraw = st->Xraw.as<double>();
    HIPCHK(hipMemcpyAsync(Xraw + npts * d, x, sizeof(double) * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(st->ybuf.as<double>() + R, yv, sizeof(double) * P, hipMemcpyHostToDevice, s));
    HIPCHK(launch_scale_points(Xraw + npts * d, st->Xs.as<double>() + npts * st->dp, 1, 1, d, st->dp, 1.0 / g->prm.ell, s));
    for (int q = 0; q < P; ++q)
        HIPCHK(launch_center(st->ybuf.as<double>() + R + q, st->delta.as<double>() + R + q, 1, 1, g->mean_vec[q], s));
    HIPCHK(hipMemsetAsync(n->info.p, 0, sizeof(int64_t), s));
    double* krow = n->Kxz.as<double>();
    double* lvec = n->tvec.as<double>();
    double* vvec = n->tvec.as<double>() + ld;
    const double* alpha_cur = g->alpha.as<double>();
    for (int q = 0; q < P; ++q) {
        const int64_t Rq = R + q;                          // rows in front of the one being appended
        KgenArgs ka = kgen_model_args(g, false);           // the old view's model (same storage, same kernel) …
        ka.N = (int)(npts + 1); ka.Np = (int)pad_up(Rq, TB); ka.rvalid = (int)Rq;      // … with the partly appended point
        ka.Z = Xraw + npts * d; ka.Kout = krow; ka.ldk = ld; ka.M = 1; ka.j0 = q; ka.Mc = 16;
        ka.pc = P; ka.point_major = 1;
        HIPCHK(launch_kgen(ka, s));
        HIPCHK(launch_trmv(st->W.as<double>(), ld, krow, lvec, (int)Rq, 1, s));
        HIPCHK(launch_trmv(st->WT.as<double>(), ld, lvec, vvec, (int)Rq, 0, s));
        double* alpha_new = (q & 1) == ((P - 1) & 1) ? n->alpha.as<double>() : n->T.as<double>();   // the last row lands in n->alpha
        AppendArgs aa{};
        aa.L = st->K.as<double>(); aa.W = st->W.as<double>(); aa.WT = st->WT.as<double>(); aa.ld = ld;
        aa.krow = krow; aa.lvec = lvec; aa.vvec = vvec; aa.alpha_old = alpha_cur; aa.alpha_new = alpha_new;
        aa.vext = n->vext.as<double>() + (int64_t)q * ld; aa.delta = st->delta.as<double>(); aa.N = (int)Rq; aa.cap = (int)ld;
        aa.kss = (q == 0 ? g->prm.sigma_f2 : grad_prior_var(g)) + st->noise_used;
        aa.scal = n->scal.as<double>() + 4 * q; aa.info = n->info.as<int64_t>();
        HIPCHK(launch_append(aa, s));
        alpha_cur = alpha_new;
    }
    double sc[4 * MAX_P];
    int64_t inf = 0;
    PinStage pin(n->ctx);
    HIPCHK(pin.d2h(sc, n->scal.p, sizeof(double) * 4 * P, s));
    HIPCHK(pin.d2h(&inf, n->info.p, sizeof inf, s));
    HIPCHK(wait_stream(s));
    pin.flush();
    if (inf != 0) {
        if (info) *info = inf;
        return fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld",
                    (long long)inf);
    }
    storage_unref(n->st);
    st->refs.fetch_add(1);
    n->st = st;
    claim.keep = true;
    n->N = R + P; n->npts = npts + 1; n->Np = pad_up(R + P, TB); n->d = d; n->dp = st->dp;
    n->from_append = true;
    n->logdet = g->logdet; n->quad = g->quad;
    for (int q = 0; q < P; ++q) {
        n->ap_s2v[q] = sc[4 * q]; n->ap_betav[q] = sc[4 * q + 1];
        n->logdet += 2.0 * std::log(sc[4 * q + 2]);
        n->quad += sc[4 * q + 1] * sc[4 * q + 1] * sc[4 * q];
    }
    n->fitted = true;
    return ABO_OK;
}

// Crossover rule of abo_remove (header): k single removals against one refit of the R − k rows that remain.  Measured with
// tools/remove_latency.py (profiles/remove_latency.txt): break-even between k = 4 and 8 for R = 1024, at k ≈ 16 for R = 8192.
int64_t remove_kmax(int64_t R) {
    const int64_t k = R / 512;
    return k < 4 ? 4 : (k > 16 ? 16 : k);
}

// View `g` (N rows) without observation j → the fresh handle `n` on a storage of its own (remove.hip; DESIGN.md "Removing an
// observation").  idx_d: j on the device.  g and its storage are only read, rows and columns < g->N of them: other views of the
// storage, larger ones included, keep their bits.  Nothing here can fail numerically: K̃ without a row and a column stays positive
// definite, and every pivot of the update is ρ_{k+1}/ρ_k ≥ 1 times the old one.
int32_t remove_one_impl(abo_gp* g, abo_gp* n, int64_t j, const int64_t* idx_d) {
    Storage* so = g->st;
    const int d = g->d;
    const int64_t N = g->N, Nn = N - 1;
    hipStream_t s = n->stream;
    Storage* st = new (std::nothrow) Storage();
    if (!st) return fail(ABO_ENOMEM, "abo_remove: host allocation failed");
    struct Drop { Storage* st; ~Drop() { if (st) storage_unref(st); } } drop{st};
    st->set_device(g->prm.device);
    st->d = d; st->dp = so->dp;
    st->cap = pad_up(g->prm.n_max > Nn ? g->prm.n_max : Nn, TB);
    const int64_t cap = st->cap, Npn = pad_up(Nn, TB);
    hipError_t e = st->Xraw.ensure(sizeof(double) * cap * d);
    if (e == hipSuccess) e = st->Xs.ensure(sizeof(double) * cap * st->dp);
    if (e == hipSuccess) e = st->ybuf.ensure(sizeof(double) * cap);
    if (e == hipSuccess) e = st->delta.ensure(sizeof(double) * cap);
    if (e == hipSuccess) e = st->K.ensure(sizeof(double) * cap * cap);
    if (e == hipSuccess) e = st->W.ensure(sizeof(double) * cap * cap);
    if (e == hipSuccess) e = st->WT.ensure(sizeof(double) * cap * cap);
    if (e == hipSuccess) e = n->alpha.ensure(sizeof(double) * cap);
    if (e == hipSuccess) e = n->tvec.ensure(sizeof(double) * cap);
    if (e == hipSuccess) e = n->info.ensure(sizeof(int64_t));
    if (e == hipSuccess) e = n->scal.ensure(sizeof(double) * 8);
    ScratchBuf work(g->prm.device, s);
    if (e == hipSuccess) e = work.b.ensure(sizeof(double) * 5 * N);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "abo_remove: device allocation failed: %s", hipGetErrorString(e));
    // what a fit leaves outside the view: zero padding of the per-point arrays and of α, zero rows with a unit diagonal behind the
    // padded size of W / WT (a later append grows into them)
    HIPCHK(hipMemsetAsync(st->Xs.p, 0, sizeof(double) * cap * st->dp, s));
    HIPCHK(hipMemsetAsync(st->delta.p, 0, sizeof(double) * cap, s));
    HIPCHK(hipMemsetAsync(n->alpha.p, 0, sizeof(double) * cap, s));
    if (cap > Npn) {
        HIPCHK(hipMemsetAsync(st->W.as<double>() + Npn * cap, 0, sizeof(double) * (cap - Npn) * cap, s));
        HIPCHK(hipMemsetAsync(st->WT.as<double>() + Npn * cap, 0, sizeof(double) * (cap - Npn) * cap, s));
        HIPCHK(launch_set_diag(st->W.as<double>(), cap, (int)Npn, (int)cap, 1.0, s));
        HIPCHK(launch_set_diag(st->WT.as<double>(), cap, (int)Npn, (int)cap, 1.0, s));
    }
    HIPCHK(launch_remove_gather(idx_d, 1, Nn, d, st->dp, so->Xraw.as<double>(), so->Xs.as<double>(), so->ybuf.as<double>(),
                                so->delta.as<double>(), st->Xraw.as<double>(), st->Xs.as<double>(), st->ybuf.as<double>(),
                                st->delta.as<double>(), s));
    RemoveArgs ra{};
    ra.L = so->K.as<double>(); ra.WT = so->WT.as<double>(); ra.alpha = g->alpha.as<double>(); ra.ld = so->cap;
    ra.Ln = st->K.as<double>(); ra.Wn = st->W.as<double>(); ra.WTn = st->WT.as<double>(); ra.alpha_n = n->alpha.as<double>();
    ra.ldn = cap; ra.N = (int)N; ra.j = (int)j; ra.work = work.b.as<double>(); ra.scal = n->scal.as<double>();
    HIPCHK(launch_remove_row(ra, s));
    double sc[3];
    PinStage pin(n->ctx);                            // the NEW handle's staging block: `g` may be in use by another thread
    HIPCHK(pin.d2h(sc, n->scal.p, sizeof sc, s));
    HIPCHK(wait_stream(s));
    pin.flush();
    const double bjj = sc[0] * sc[0] * sc[1];        // B_jj = (K̃⁻¹)_jj = ω²·ρ_m²
    st->noise_used = so->noise_used;
    st->add_view(Nn);
    drop.st = nullptr;
    storage_unref(n->st);
    n->st = st;
    n->N = Nn; n->npts = Nn; n->Np = Npn; n->d = d; n->dp = st->dp;
    n->from_append = false;
    n->ap_x.clear();
    n->logdet = g->logdet + std::log(bjj);
    n->quad = g->quad - sc[2] * sc[2] / bjj;
    n->fitted = true;
    return ABO_OK;
}

// Blocked bordered update (append_batch.hip): view `g` (N points) → new view `n` (N + k points, 1 ≤ k ≤ 64) sharing g's
// storage, in one step.  Xd / yd: the k points and targets on the DEVICE, followed by the rest − k that the caller will append next:
// when the rows cannot be claimed (capacity used up, or another view appended past g) all `rest` are gathered behind g's data and
// refitted, as append_impl falls back (*refitted = true).  One host read-back: info and the two scalars.
int32_t append_batch_step(abo_gp* g, abo_gp* n, const double* Xd, const double* yd, int k, int64_t rest, int64_t* info, bool* refitted) {
    Storage* st = g->st;
    const int d = g->d;
    const int64_t N = g->N;
    hipStream_t s = n->stream;
    *refitted = false;
    // (all `rest` points must fit, not this step's alone: a batch of several steps that will not fit goes straight to the refit)
    if (N + rest > st->cap || !st->claim_rows(N, N + k)) {
        const int64_t Nn = N + rest;
        ScratchBuf xs(g->prm.device, s), ys(g->prm.device, s);
        HIPCHK(xs.b.ensure(sizeof(double) * Nn * d));
        HIPCHK(ys.b.ensure(sizeof(double) * Nn));
        HIPCHK(hipMemcpyAsync(xs.b.p, st->Xraw.p, sizeof(double) * N * d, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ys.b.p, st->ybuf.p, sizeof(double) * N, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(xs.b.as<double>() + N * d, Xd, sizeof(double) * rest * d, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(ys.b.as<double>() + N, yd, sizeof(double) * rest, hipMemcpyDeviceToDevice, s));
        HIPCHK(wait_stream(s));
        if (n->prm.n_max < 2 * Nn) n->prm.n_max = 2 * Nn;
        *refitted = true;
        return fit_impl(n, xs.b.as<double>(), Nn, d, ys.b.as<double>(), ABO_DEVICE, info);
    }
    // rows [N, N + k) are claimed: every failure below gives them back
    struct Claim { Storage* st; int64_t n; bool keep = false; ~Claim() { if (!keep) st->drop_view(n); } } claim{st, N + k};
    const int64_t ld = st->cap;
    const int kp = (int)pad_up(k, 16);
    const int64_t Npk = pad_up(N + k, TB);
    const int G = append_batch_gram_blocks((int)N);
    HIPCHK(n->alpha.ensure(sizeof(double) * ld));
    HIPCHK(n->info.ensure(sizeof(int64_t)));
    HIPCHK(n->scal.ensure(sizeof(double) * 8));
    // scratch of the step: K_b with K_bb behind it, B, C, the slice sums of a block product, the Gram sums, {L_s, L_s⁻¹, β} — about
    // 11·N·kp doubles, 8 of the 11 being the slice sums: 92 MB at N = 16384, k = 64 (5.8 MB at N = 8192, k = 8); from the pool, back
    // to it when the step returns
    const size_t nkb = (size_t)(N + kp) * kp, nb = (size_t)N * kp, npart = tri_skinny_part_doubles((int)N, kp);
    const size_t ngram = (size_t)G * (kp * kp + kp), nsm = (size_t)2 * kp * kp + kp;
    ScratchBuf work(g->prm.device, s);
    HIPCHK(work.b.ensure(sizeof(double) * (nkb + 2 * nb + npart + ngram + nsm)));
    double* Kb = work.b.as<double>();
    double* Bm = Kb + nkb;
    double* Cm = Bm + nb;
    double* part = Cm + nb;
    double* gpart = part + npart;
    double* sm = gpart + ngram;
    double* Xraw = st->Xraw.as<double>();
    const double sc_ell = 1.0 / g->prm.ell;
    HIPCHK(launch_append_batch_points(Xd, yd, k, d, st->dp, sc_ell, g->prm.mean_c, Xraw + N * d, st->Xs.as<double>() + N * st->dp,
                                      st->ybuf.as<double>() + N, st->delta.as<double>() + N, n->info.as<int64_t>(), s));
    HIPCHK(launch_append_batch_newcols(st->Xs.as<double>() + N * st->dp, Xraw, Kb, (int)N, k, d, st->dp, g->prm.family, sc_ell,
                                       g->prm.sigma_f2, s));
    // only rows / columns < N of W and WT: anything beyond may be the stale remains of a discarded branch
    tl_phase_np = Npk;
    const bool timed = phase_events();
    // (scratch slots EV_BASE + 0 … 3: begin and end of each block product — the k × k part runs between them)
    if (timed) { HIPCHK(n->events(EV_BASE + 4)); HIPCHK(hipEventRecord(n->evs()[EV_BASE], s)); }
    HIPCHK(launch_tri_skinny(st->W.as<double>(), ld, Kb, Bm, part, (int)N, kp, 1, s));
    if (timed) HIPCHK(hipEventRecord(n->evs()[EV_BASE + 1], s));
    HIPCHK(launch_append_batch_small(Bm, Kb, g->alpha.as<double>(), st->delta.as<double>() + N, (int)N, k, st->noise_used, gpart, sm,
                                     n->scal.as<double>(), n->info.as<int64_t>(), s));
    if (timed) HIPCHK(hipEventRecord(n->evs()[EV_BASE + 2], s));
    HIPCHK(launch_tri_skinny(st->WT.as<double>(), ld, Bm, Cm, part, (int)N, kp, 0, s));
    if (timed) HIPCHK(hipEventRecord(n->evs()[EV_BASE + 3], s));
    AppendBatchArgs wa{};
    wa.L = st->K.as<double>(); wa.W = st->W.as<double>(); wa.WT = st->WT.as<double>(); wa.ld = ld; wa.B = Bm; wa.C = Cm; wa.sm = sm;
    wa.alpha_old = g->alpha.as<double>(); wa.alpha_new = n->alpha.as<double>(); wa.N = N; wa.cap = ld; wa.k = k; wa.kp = kp;
    wa.info = n->info.as<int64_t>();
    HIPCHK(launch_append_batch_write(wa, s));
    double sc[2] = {0.0, 0.0};
    int64_t inf = 0;
    PinStage pin(n->ctx);                            // the NEW handle's staging block: `g` may be in use by another thread
    HIPCHK(pin.d2h(sc, n->scal.p, sizeof sc, s));
    HIPCHK(pin.d2h(&inf, n->info.p, sizeof inf, s));
    HIPCHK(wait_stream(s));
    pin.flush();
    if (inf != 0) {
        if (info) *info = inf;
        return fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld",
                    (long long)inf);
    }
    storage_unref(n->st);
    st->refs.fetch_add(1);
    n->st = st;
    claim.keep = true;                               // (registered by claim_rows)
    n->N = N + k; n->npts = N + k; n->Np = Npk; n->d = d; n->dp = st->dp;
    // an appended view, but of no ONE-row append: no down-date vector (vext stays unallocated), no appended point — abo_cand_downdate
    // and abo_paths_append (gp_append_view) refuse a view without them, whatever the set or the paths were last synced with
    n->from_append = true;
    n->ap_x.clear();
    n->ap_serial = g_append_serial.fetch_add(1);
    n->ap_s2 = 0.0; n->ap_beta = 0.0;
    // the two block products B = L⁻¹K_b, C = L⁻ᵀB: each streams one triangle of its matrix once (8·N²/2 bytes), whatever k
    n->tm.append_trmv_ms = timed ? ev_ms(n->evs()[EV_BASE], n->evs()[EV_BASE + 1]) + ev_ms(n->evs()[EV_BASE + 2], n->evs()[EV_BASE + 3]) : 0.0;
    n->tm.append_trmv_bytes = 8.0 * (double)N * (double)N;
    n->logdet = g->logdet + sc[0];
    n->quad = g->quad + sc[1];
    n->fitted = true;
    return ABO_OK;
}

}  // namespace

extern "C" {

int32_t abo_abi_version(void) { return ABO_ABI_VERSION; }

int32_t abo_last_error(char* buf, size_t cap) {
    if (!buf || cap == 0) return ABO_EINVAL;
    strncpy(buf, g_err, cap - 1);
    buf[cap - 1] = '\0';
    return ABO_OK;
}

int32_t abo_create(const abo_params* params, abo_gp** out) {
    if (!params || !out) return fail(ABO_EINVAL, "abo_create: null argument");
    if (params->family < ABO_KERNEL_SE || params->family > ABO_KERNEL_MATERN32)
        return fail(ABO_EINVAL, "abo_create: unknown kernel family %d", params->family);
    if (!(params->ell > 0.0) || !(params->sigma_f2 > 0.0) || !(params->noise_var >= 0.0) || !(params->jitter >= 0.0) ||
        !std::isfinite(params->mean_c))
        return fail(ABO_EINVAL, "abo_create: need ell > 0, sigma_f2 > 0, noise_var >= 0, jitter >= 0, finite mean");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (params->device < 0 || params->device >= ndev)
        return fail(ABO_EINVAL, "abo_create: device %d not present (%d devices)", params->device, ndev);
    HIPCHK(hipSetDevice(params->device));
    abo::arm_exit_guard();
    abo_gp* g = new (std::nothrow) abo_gp();
    if (!g) return fail(ABO_ENOMEM, "abo_create: host allocation failed");
    g->prm = *params;
    g->mean_vec[0] = params->mean_c;
    g->set_device(params->device);
    oz_defaults(&g->oz_engine, &g->oz_nmod);
    {
        std::lock_guard<std::mutex> lk(g_ctx_mu);
        auto& fl = g_ctx_free[params->device & 15];
        if (!fl.empty()) { g->ctx = fl.back(); fl.pop_back(); }
    }
    hipError_t e = hipSuccess;
    if (!g->ctx) {
        g->ctx = new (std::nothrow) ExecCtx();
        if (!g->ctx) { delete g; return fail(ABO_ENOMEM, "abo_create: host allocation failed"); }
        e = hipStreamCreateWithFlags(&g->ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete g->ctx; delete g; return fail(ABO_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
        void* pin = nullptr;                               // optional: without it the small read-backs go to pageable memory as before
        static const bool no_pin = getenv("ABO_NO_PINNED") != nullptr;         // A/B and the test of the fallback
        if (!no_pin && hipHostMalloc(&pin, PIN_BYTES, hipHostMallocDefault) == hipSuccess) g->ctx->pin = static_cast<char*>(pin);
        else (void)hipGetLastError();
    }
    g->stream = g->ctx->stream;
    e = g->events(EV_ACQ_END + 1);
    if (e != hipSuccess) { g->free_all(); delete g; return fail(ABO_EHIP, "hipEventCreate: %s", hipGetErrorString(e)); }
    *out = g;
    return ABO_OK;
}

int32_t abo_create_grad(const abo_params* params, int32_t p, const double* mean_c, abo_gp** out) {
    if (!params || !out) return fail(ABO_EINVAL, "abo_create_grad: null argument");
    if (p < 2 || p > MAX_P)
        return fail(ABO_EINVAL, "abo_create_grad: p = %d outputs outside 2..%d (library limit: a gradient-enhanced GP has "
                                "d = p − 1 ≤ %d inputs)", p, MAX_P, MAX_P - 1);
    if (params->family != ABO_KERNEL_SE && params->family != ABO_KERNEL_MATERN52 && params->family != ABO_KERNEL_MATERN72)
        return fail(ABO_EINVAL, "abo_create_grad: the gradient-enhanced GP needs a twice-differentiable kernel "
                                "(SE, Matern-5/2, Matern-7/2)");
    int32_t rc = abo_create(params, out);
    if (rc) return rc;
    (*out)->p_out = p;
    for (int q = 0; q < p; ++q) {
        const double c = mean_c ? mean_c[q] : 0.0;
        if (!std::isfinite(c)) { abo_destroy(*out); *out = nullptr; return fail(ABO_EINVAL, "abo_create_grad: non-finite mean"); }
        (*out)->mean_vec[q] = c;
    }
    return ABO_OK;
}

int32_t abo_set_contraction(abo_gp* gp, int32_t engine, int32_t nmod) {
    if (engine < ABO_CONTRACT_AUTO || engine > ABO_CONTRACT_INT8) return fail(ABO_EINVAL, "abo_set_contraction: unknown engine %d", engine);
    if (nmod != 0 && (nmod < 8 || nmod > OZ_MAXMOD)) return fail(ABO_EINVAL, "abo_set_contraction: 8 to %d moduli (0 = default)", OZ_MAXMOD);
    if (!gp) {
        int e, n;
        oz_defaults(&e, &n);
        g_oz_nmod.store(nmod ? nmod : OZ_DEFAULT_NMOD);
        g_oz_engine.store(engine);
        return ABO_OK;
    }
    gp->oz_engine = engine;
    gp->oz_nmod = nmod;                                            // 0: whatever the process default is when the posterior runs
    return ABO_OK;
}

int32_t abo_retain(abo_gp* gp) {
    if (!gp) return fail(ABO_EINVAL, "null handle");
    gp->refs.fetch_add(1);
    return ABO_OK;
}

int32_t abo_destroy(abo_gp* gp) {
    if (!gp) return ABO_OK;
    // a finaliser that fires while the process exits (or after the runtime reported itself gone): the handle's device state
    // is reclaimed with the process — nothing here may call into HIP any more, and nothing is worth freeing
    if (g_exiting.load()) return ABO_OK;
    if (gp->refs.fetch_sub(1) == 1) {
        hipError_t e = hipSetDevice(gp->prm.device);
        if (e == hipSuccess && gp->stream) e = wait_stream(gp->stream);
        if (abo::gone(e)) { g_exiting.store(true); return ABO_OK; }      // the runtime says it has been torn down: the process is exiting
        // any other error of these two calls concerns this handle only: its buffers still go back to the pool, nothing is latched
        (void)hipGetLastError();
        gp->free_all();
        delete gp;
    }
    return ABO_OK;
}

int32_t abo_fit(abo_gp* g, const double* X, int64_t N, int32_t d, const double* y, int32_t space, int64_t* info) {
    if (info) *info = 0;
    if (!g || !X || !y) return fail(ABO_EINVAL, "abo_fit: null argument");
    if (N < 1) return fail(ABO_EINVAL, "abo_fit: need at least one training point");
    if (d < 1 || d > 65536) return fail(ABO_EINVAL, "abo_fit: input dimension %d outside 1..65536", d);
    if (N > (int64_t)1 << 20) return fail(ABO_EINVAL, "abo_fit: N = %lld too large", (long long)N);
    if (g->p_out > 1 && d + 1 != g->p_out)
        return fail(ABO_EDIM, "DimensionMismatch: gradient-enhanced model with p = %d outputs needs d = %d inputs, got %d",
                    g->p_out, g->p_out - 1, d);
    HIPCHK(hipSetDevice(g->prm.device));
    return fit_impl(g, X, N, d, y, space, info);
}

int32_t abo_append(abo_gp* g, const double* x, int32_t d, double y, int64_t* info, abo_gp** out) {
    if (info) *info = 0;
    if (!g || !x || !out) return fail(ABO_EINVAL, "abo_append: null argument");
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (g->p_out > 1) return fail(ABO_EINVAL, "abo_append: a gradient-enhanced model takes p values per observation (abo_append_grad)");
    HIPCHK(hipSetDevice(g->prm.device));
    abo_gp* n = nullptr;
    rc = abo_create(&g->prm, &n);
    if (rc) return rc;
    n->oz_engine = g->oz_engine; n->oz_nmod = g->oz_nmod;
    rc = append_impl(g, n, x, y, info);
    if (rc) { abo_destroy(n); return rc; }
    *out = n;
    return ABO_OK;
}

int32_t abo_append_grad(abo_gp* g, const double* x, int32_t d, const double* y, int64_t* info, abo_gp** out) {
    if (info) *info = 0;
    if (!g || !x || !y || !out) return fail(ABO_EINVAL, "abo_append_grad: null argument");
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (g->p_out < 2) return fail(ABO_EINVAL, "abo_append_grad: the model has no gradient outputs (abo_append)");
    HIPCHK(hipSetDevice(g->prm.device));
    abo_gp* n = nullptr;
    rc = abo_create(&g->prm, &n);
    if (rc) return rc;
    n->p_out = g->p_out;
    n->oz_engine = g->oz_engine; n->oz_nmod = g->oz_nmod;
    for (int q = 0; q < MAX_P; ++q) n->mean_vec[q] = g->mean_vec[q];
    rc = append_grad_impl(g, n, x, y, info);
    if (rc) { abo_destroy(n); return rc; }
    *out = n;
    return ABO_OK;
}

int32_t abo_append_batch(abo_gp* g, const double* X, int32_t k, int32_t d, const double* y, int32_t space, int64_t* info, abo_gp** out) {
    if (info) *info = 0;
    if (!g || !X || !y || !out) return fail(ABO_EINVAL, "abo_append_batch: null argument");
    if (k < 1) return fail(ABO_EINVAL, "abo_append_batch: k = %d, need at least one point", k);
    if (space != ABO_HOST && space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_append_batch: unknown memory space %d", space);
    if (!g->fitted) return fail(ABO_EINVAL, "abo_append_batch: surrogate is not conditioned on data yet (call abo_fit first)");
    if (g->p_out > 1)
        return fail(ABO_EINVAL, "abo_append_batch: gradient-enhanced models are not supported (abo_append_grad, one observation at a time)");
    if (d != g->d) return fail(ABO_EINVAL, "abo_append_batch: point dimension %d, model dimension %d", d, g->d);
    if (g->N + (int64_t)k > (int64_t)1 << 20) return fail(ABO_EINVAL, "abo_append_batch: N + k = %lld too large", (long long)(g->N + k));
    tl_phase_np = g->Np;
    HIPCHK(hipSetDevice(g->prm.device));
    abo_gp* n = nullptr;
    int32_t rc = abo_create(&g->prm, &n);
    if (rc) return rc;
    n->oz_engine = g->oz_engine; n->oz_nmod = g->oz_nmod;
    if (k == 1) {                                    // abo_append's own path, bit for bit: the view abo_cand_downdate / abo_paths_append follow
        std::vector<double> xh(X, X + (space == ABO_HOST ? d : 0));
        double yh = space == ABO_HOST ? y[0] : 0.0;
        if (space == ABO_DEVICE) {
            xh.resize(d);
            hipError_t e = hipMemcpyAsync(xh.data(), X, sizeof(double) * d, hipMemcpyDeviceToHost, n->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&yh, y, sizeof(double), hipMemcpyDeviceToHost, n->stream);
            if (e == hipSuccess) e = wait_stream(n->stream);
            if (e != hipSuccess) { abo_destroy(n); return fail(ABO_EHIP, "abo_append_batch: reading the point failed: %s", hipGetErrorString(e)); }
        }
        rc = append_impl(g, n, xh.data(), yh, info);
        if (rc) { abo_destroy(n); return rc; }
        *out = n;
        return ABO_OK;
    }
    // the points on the device (host arrays: staged once for every step; the caller's arrays are free again when the call returns)
    ScratchBuf stage(g->prm.device, n->stream);
    const double* Xd = X;
    const double* yd = y;
    if (space == ABO_HOST) {
        hipError_t e = stage.b.ensure(sizeof(double) * (size_t)k * (d + 1));
        if (e == hipSuccess) e = hipMemcpyAsync(stage.b.p, X, sizeof(double) * (size_t)k * d, hipMemcpyHostToDevice, n->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(stage.b.as<double>() + (size_t)k * d, y, sizeof(double) * (size_t)k, hipMemcpyHostToDevice, n->stream);
        if (e == hipSuccess) e = wait_stream(n->stream);
        if (e != hipSuccess) {
            abo_destroy(n);
            return fail(e == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "abo_append_batch: staging the points failed: %s", hipGetErrorString(e));
        }
        Xd = stage.b.as<double>();
        yd = Xd + (size_t)k * d;
    }
    // successive blocked steps of at most 64 rows; an intermediate view goes back with its handle (its rows with it on failure)
    abo_gp* cur = g;
    double trmv_ms = 0.0, trmv_bytes = 0.0;
    for (int32_t done = 0; done < k;) {
        if (!n) {
            rc = abo_create(&g->prm, &n);
            if (rc) { if (cur != g) abo_destroy(cur); return rc; }
            n->oz_engine = g->oz_engine; n->oz_nmod = g->oz_nmod;
        }
        const int kc = k - done < APPEND_BATCH_MAX ? k - done : APPEND_BATCH_MAX;
        bool refitted = false;
        rc = append_batch_step(cur, n, Xd + (size_t)done * d, yd + done, kc, k - done, info, &refitted);
        if (cur != g) abo_destroy(cur);
        if (rc) { abo_destroy(n); return rc; }
        if (refitted) {
            done = k;
        } else {
            done += kc;
            trmv_ms += n->tm.append_trmv_ms; trmv_bytes += n->tm.append_trmv_bytes;
            n->tm.append_trmv_ms = trmv_ms; n->tm.append_trmv_bytes = trmv_bytes;
        }
        cur = n;
        n = nullptr;
    }
    *out = cur;
    return ABO_OK;
}

int32_t abo_remove(abo_gp* g, const int64_t* idx, int32_t k, int32_t* path, abo_gp** out) {
    if (path) *path = ABO_REMOVE_REFIT;
    if (!g || !idx || !out) return fail(ABO_EINVAL, "abo_remove: null argument");
    if (k < 1) return fail(ABO_EINVAL, "abo_remove: k = %d, need at least one index", k);
    if (!g->fitted) return fail(ABO_EINVAL, "abo_remove: surrogate is not conditioned on data yet (call abo_fit first)");
    if (g->p_out > 1) return fail(ABO_EINVAL, "abo_remove: gradient-enhanced models are not supported (refit on the remaining points)");
    const int64_t N = g->N;
    for (int32_t t = 0; t < k; ++t) {
        if (idx[t] < 0 || idx[t] >= N) return fail(ABO_EINVAL, "abo_remove: index %lld outside 0..%lld", (long long)idx[t], (long long)N - 1);
        if (t > 0 && idx[t] <= idx[t - 1]) return fail(ABO_EINVAL, "abo_remove: indices must be strictly increasing (no duplicates)");
    }
    if (N - k < 1) return fail(ABO_EINVAL, "abo_remove: removing %d of %lld points leaves none", k, (long long)N);
    HIPCHK(hipSetDevice(g->prm.device));
    abo_gp* n = nullptr;
    int32_t rc = abo_create(&g->prm, &n);
    if (rc) return rc;
    n->oz_engine = g->oz_engine; n->oz_nmod = g->oz_nmod;
    hipStream_t s = n->stream;
    const int d = g->d;
    const int64_t Nn = N - k;
    const bool refit = k > remove_kmax(N);
    // the indices on the device, and (refit) the points and targets that remain
    ScratchBuf buf(g->prm.device, s);
    const size_t idx_bytes = (sizeof(int64_t) * (size_t)k + 15) & ~(size_t)15;
    hipError_t e = buf.b.ensure(idx_bytes + (refit ? sizeof(double) * (size_t)Nn * (d + 1) : 0));
    if (e != hipSuccess) {
        abo_destroy(n);
        return fail(e == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "abo_remove: device allocation failed: %s", hipGetErrorString(e));
    }
    int64_t* idx_d = buf.b.as<int64_t>();
    e = hipMemcpyAsync(idx_d, idx, sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = wait_stream(s);          // the caller's array is free again when the call returns, whatever happens below
    if (e != hipSuccess) { abo_destroy(n); return fail(ABO_EHIP, "abo_remove: staging the indices failed: %s", hipGetErrorString(e)); }
    if (refit) {
        Storage* so = g->st;
        double* xb = reinterpret_cast<double*>(buf.b.as<char>() + idx_bytes);
        double* yb = xb + (size_t)Nn * d;
        e = launch_remove_gather(idx_d, k, Nn, d, so->dp, so->Xraw.as<double>(), nullptr, so->ybuf.as<double>(), nullptr, xb, nullptr, yb,
                                 nullptr, s);
        if (e != hipSuccess) { abo_destroy(n); return fail(ABO_EHIP, "abo_remove: gather launch failed: %s", hipGetErrorString(e)); }
        int64_t inf = 0;
        rc = fit_impl(n, xb, Nn, d, yb, ABO_DEVICE, &inf);
        if (rc) { abo_destroy(n); return rc; }
        *out = n;
        return ABO_OK;
    }
    // k single removals, highest index first (the lower ones keep their positions), each into a storage of its own: the one before
    // goes back to the pool with its handle, so two storages alternate
    abo_gp* cur = g;
    for (int32_t t = k - 1; t >= 0; --t) {
        if (!n) {
            rc = abo_create(&g->prm, &n);
            if (rc) { if (cur != g) abo_destroy(cur); return rc; }
            n->oz_engine = g->oz_engine; n->oz_nmod = g->oz_nmod;
        }
        rc = remove_one_impl(cur, n, idx[t], idx_d + t);
        if (cur != g) abo_destroy(cur);
        if (rc) { abo_destroy(n); return rc; }
        cur = n;
        n = nullptr;
    }
    if (path) *path = ABO_REMOVE_REMOVED;
    *out = cur;
    return ABO_OK;
}

}  // extern "C"

namespace {
// after the synchronisation that followed a deferred fit: the verdict on the factorisation
int32_t fit_finish(abo_gp* g, int64_t* info) {
    if (g->h_info() != 0) {
        if (g->st && g->fitted) g->st->drop_view(g->N);
        g->fitted = false;
        if (info) *info = g->h_info();
        return fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld",
                    (long long)g->h_info());
    }
    fit_collect(g);
    return ABO_OK;
}
}  // namespace

extern "C" {

int32_t abo_fit_acq(abo_gp* g, const double* X, int64_t N, int32_t d, const double* y, int32_t space, int64_t* info, const double* Z,
                    int64_t M, int32_t z_space, int32_t kind, double p0, double best_y, int64_t idx_base, double* scores, int32_t k,
                    double* top_val, int64_t* top_idx, int32_t out_space) {
    if (info) *info = 0;
    if (!g || !X || !y) return fail(ABO_EINVAL, "abo_fit_acq: null argument");
    // an opt-in jitter retry needs the verdict on the factorisation before anything else is queued, and a gradient-enhanced
    // model's targets are reordered on the way in: both take the two calls this entry point otherwise fuses
    if (g->prm.jitter > 0.0 || g->p_out > 1) {
        const int32_t rc = abo_fit(g, X, N, d, y, space, info);
        return rc ? rc : abo_acq(g, Z, M, d, z_space, kind, p0, best_y, idx_base, scores, k, top_val, top_idx, out_space);
    }
    if (N < 1) return fail(ABO_EINVAL, "abo_fit_acq: need at least one training point");
    if (d < 1 || d > 65536) return fail(ABO_EINVAL, "abo_fit_acq: input dimension %d outside 1..65536", d);
    if (N > (int64_t)1 << 20) return fail(ABO_EINVAL, "abo_fit_acq: N = %lld too large", (long long)N);
    HIPCHK(hipSetDevice(g->prm.device));
    int32_t rc = fit_impl(g, X, N, d, y, space, info, 0, /*defer=*/true);
    if (rc) return rc;
    // the acquisition's launches go straight behind the fit's: after a failed pivot they work on finite leftovers or exit on
    // `info`, and their results are discarded below
    rc = abo::acq_ex(g, Z, M, d, z_space, kind, p0, best_y, idx_base, scores, out_space, k, top_val, top_idx, out_space);
    if (rc) { (void)wait_stream(g->stream); (void)fit_finish(g, info); return rc; }
    return fit_finish(g, info);           // acq_ex returned behind its stream synchronisation: the fit's scalars have landed
}

int32_t abo_nlml(abo_gp* g, double* out) {
    if (!g || !out) return fail(ABO_EINVAL, "abo_nlml: null argument");
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    *out = 0.5 * ((double)g->N * std::log(2.0 * M_PI) + g->logdet + g->quad);
    return ABO_OK;
}

// abo_nlml_grad and abo_nlml_grad_ard behind their argument checks: K⁻¹ = WᵀW, the trace sweep (one ∂/∂log ℓ, or ard = one per
// coordinate into d_log_ell[0 … d)), the scalars both derive from the finish step's sums
static int32_t nlml_grad_impl(abo_gp* g, bool ard, double* nlml, double* d_log_ell, double* d_log_sigma_f2, double* d_log_noise) {
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const int64_t Np = g->Np, ld = g->st->cap;
    const int N = (int)g->N;
    HIPCHK(g->T.ensure(sizeof(double) * Np * Np));
    const int64_t npart = ard ? Np / 16 * g->dp : Np / 16;       // ard: partial[block][c], the dp reduced traces behind them
    HIPCHK(g->partial.ensure(sizeof(double) * (npart + (ard ? g->dp : 0) + 8)));
    HIPCHK(g->scal.ensure(sizeof(double) * 8));
    // K⁻¹ = WᵀW on the lower 128-tiles: Kinv[i][j] = Σ_{k ≥ i} WT[i][k]·WT[j][k]
    GemmArgs a{};
    a.A = g->st->WT.as<double>(); a.lda = ld; a.B = g->st->WT.as<double>(); a.ldb = ld;
    a.C = g->T.as<double>(); a.ldc = Np; a.M = (int)Np; a.N = (int)Np; a.K = (int)Np;
    a.kmode = K_A_UPPER; a.lower_only = 1; a.batch = 1; a.alpha = 1.0; a.beta = 0.0;
    HIPCHK(g->events(EV_BASE + 3));
    hipEvent_t* ev = &g->evs()[EV_BASE];          // scratch slots: ev[0] begin, ev[1] K⁻¹ formed, ev[2] traces done (no posterior pass in this call)
    HIPCHK(hipEventRecord(ev[0], s));
    HIPCHK(launch_gemm_nt(a, s));
    HIPCHK(hipEventRecord(ev[1], s));
    NlmlGradArgs ga{};
    ga.Xs = g->st->Xs.as<double>(); ga.Kinv = g->T.as<double>(); ga.alpha = g->alpha.as<double>();
    ga.delta = g->st->delta.as<double>(); ga.partial = g->partial.as<double>(); ga.out = g->scal.as<double>() + 4;
    ga.ld = Np; ga.N = N; ga.Np = (int)Np; ga.dp = g->dp; ga.family = g->prm.family; ga.sigma_f2 = g->prm.sigma_f2;
    if (ard) {
        HIPCHK(launch_nlml_grad_ard(ga, g->partial.as<double>() + npart, s));
    } else if (g->p_out > 1) {
        // gradient-enhanced GP: dK/dlog(ell) of the multi-output system as a matrix (same generator as K_XX with the
        // derivative triple), then the weighted sum against K^-1 - alpha alpha^T
        HIPCHK(g->Kxz.ensure(sizeof(double) * Np * Np));
        KgenArgs ka = kgen_model_args(g, false);
        ka.Z = g->st->Xraw.as<double>(); ka.Kout = g->Kxz.as<double>(); ka.ldk = Np; ka.M = g->npts; ka.Mc = (int)Np;
        ka.pc = g->p_out; ka.point_major = 1; ka.dlogell = 1;
        HIPCHK(launch_kgen(ka, s));
        HIPCHK(launch_nlml_grad_matrix(ga, g->Kxz.as<double>(), Np, s));
    } else {
        HIPCHK(launch_nlml_grad(ga, s));
    }
    HIPCHK(hipEventRecord(ev[2], s));
    double o[4], oc[32];
    HIPCHK(hipMemcpyAsync(o, g->scal.as<double>() + 4, sizeof o, hipMemcpyDeviceToHost, s));
    if (ard) HIPCHK(hipMemcpyAsync(oc, g->partial.as<double>() + npart, sizeof(double) * g->d, hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    g->tm.nlml_kinv_ms = ev_ms(ev[0], ev[1]);
    g->tm.nlml_trace_ms = ev_ms(ev[1], ev[2]);
    // ∂NLML/∂θ = ½ tr((K⁻¹ − ααᵀ) ∂K/∂θ);  ∂K/∂log σ_f² = K − noise·I  and  K α = δ
    const double noise = g->st->noise_used;
    if (nlml) *nlml = 0.5 * ((double)g->N * std::log(2.0 * M_PI) + g->logdet + g->quad);
    if (d_log_ell) {
        if (ard) for (int c = 0; c < g->d; ++c) d_log_ell[c] = 0.5 * oc[c];
        else *d_log_ell = 0.5 * o[0];
    }
    if (d_log_sigma_f2) *d_log_sigma_f2 = 0.5 * ((double)N - noise * o[1] - o[3] + noise * o[2]);
    if (d_log_noise) *d_log_noise = 0.5 * noise * (o[1] - o[2]);      // ∂K/∂log σ² = σ²·I
    return ABO_OK;
}

int32_t abo_nlml_grad(abo_gp* g, double* nlml, double* d_log_ell, double* d_log_sigma_f2) {
    if (!g) return fail(ABO_EINVAL, "abo_nlml_grad: null handle");
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    if (g->from_append || g->st->max_live() != g->N)
        return fail(ABO_EINVAL, "abo_nlml_grad needs a freshly fitted model (hyper-parameter search refits anyway)");
    return nlml_grad_impl(g, false, nlml, d_log_ell, d_log_sigma_f2, nullptr);
}

int32_t abo_nlml_grad_ard(abo_gp* g, int32_t d, double* nlml, double* d_log_ell, double* d_log_sigma_f2, double* d_log_noise) {
    if (!g) return fail(ABO_EINVAL, "abo_nlml_grad_ard: null handle");
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    if (d < 1 || d > 32) return fail(ABO_EINVAL, "abo_nlml_grad_ard: input dimension %d outside 1..32", d);
    if (g->p_out > 1) return fail(ABO_EINVAL, "abo_nlml_grad_ard: gradient-enhanced models have no per-coordinate length scales");
    if (d != g->d) return fail(ABO_EDIM, "DimensionMismatch: abo_nlml_grad_ard with d = %d, model dimension %d", d, g->d);
    if (g->from_append || g->st->max_live() != g->N)
        return fail(ABO_EINVAL, "abo_nlml_grad_ard needs a freshly fitted model (hyper-parameter search refits anyway)");
    return nlml_grad_impl(g, true, nlml, d_log_ell, d_log_sigma_f2, d_log_noise);
}

// what abo_loo and abo_loo_grad check alike, before any device work
static int32_t loo_check(abo_gp* g, const char* who) {
    if (!g) return fail(ABO_EINVAL, "%s: null handle", who);
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    if (g->p_out > 1) return fail(ABO_EINVAL, "%s: leaving out one output row of a gradient-enhanced point is not leave-one-out", who);
    return ABO_OK;
}

// abo_loo behind its argument checks, and the value of abo_loo_grad (one implementation: the same bits): the view's own N rows of the
// triangle of WT, read once
static int32_t loo_value_impl(abo_gp* g, double* mu, double* var, double* lpd, double* nlpl, int32_t out_space) {
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const int N = (int)g->N;
    const bool host = out_space != ABO_DEVICE;
    LooArgs a{};
    a.WT = g->st->WT.as<double>(); a.ld = g->st->cap; a.alpha = g->alpha.as<double>(); a.delta = g->st->delta.as<double>();
    a.N = N; a.mean_c = g->prm.mean_c;
    const int nb = loo_diag_blocks(N);
    HIPCHK(g->partial.ensure(sizeof(double) * (nb + 8)));
    a.partial = g->partial.as<double>(); a.nlpl = a.partial + nb;          // the sum lands behind the partials
    if (mu) { if (host) { HIPCHK(g->mu_all.ensure(sizeof(double) * N)); a.mu = g->mu_all.as<double>(); } else a.mu = mu; }
    if (var) { if (host) { HIPCHK(g->var_all.ensure(sizeof(double) * N)); a.var = g->var_all.as<double>(); } else a.var = var; }
    if (lpd) { if (host) { HIPCHK(g->score_all.ensure(sizeof(double) * N)); a.lpd = g->score_all.as<double>(); } else a.lpd = lpd; }
    HIPCHK(launch_loo_diag(a, s));
    if (host) {
        if (mu) HIPCHK(hipMemcpyAsync(mu, a.mu, sizeof(double) * N, hipMemcpyDeviceToHost, s));
        if (var) HIPCHK(hipMemcpyAsync(var, a.var, sizeof(double) * N, hipMemcpyDeviceToHost, s));
        if (lpd) HIPCHK(hipMemcpyAsync(lpd, a.lpd, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    }
    double v = 0.0;
    if (nlpl) HIPCHK(hipMemcpyAsync(&v, a.nlpl, sizeof v, hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    if (nlpl) *nlpl = v;
    return ABO_OK;
}

int32_t abo_loo(abo_gp* g, double* mu, double* var, double* lpd, double* nlpl, int32_t out_space) {
    if (const int32_t rc = loo_check(g, "abo_loo")) return rc;
    if (out_space != ABO_HOST && out_space != ABO_DEVICE) return fail(ABO_EINVAL, "abo_loo: out_space %d is neither ABO_HOST nor ABO_DEVICE", out_space);
    return loo_value_impl(g, mu, var, lpd, nlpl, out_space);
}

int32_t abo_loo_grad(abo_gp* g, double* nlpl, double* d_log_ell, double* d_log_sigma_f2, double* d_log_noise) {
    if (const int32_t rc = loo_check(g, "abo_loo_grad")) return rc;
    if (g->from_append || g->st->max_live() != g->N)
        return fail(ABO_EINVAL, "abo_loo_grad needs a freshly fitted model (hyper-parameter search refits anyway)");
    if (const int32_t rc = loo_value_impl(g, nullptr, nullptr, nullptr, nlpl, ABO_HOST)) return rc;
    if (!d_log_ell && !d_log_sigma_f2 && !d_log_noise) return ABO_OK;
    hipStream_t s = g->stream;
    const int64_t Np = g->Np, ld = g->st->cap;
    const int N = (int)g->N;
    HIPCHK(g->T.ensure(sizeof(double) * Np * Np));
    HIPCHK(g->Kxz.ensure(sizeof(double) * Np * Np));
    HIPCHK(g->loo_T.ensure(sizeof(double) * Np * Np));
    const int nb = loo_grad_blocks(N);
    HIPCHK(g->partial.ensure(sizeof(double) * (3 * (size_t)nb + 8)));
    // B = K̃⁻¹ = WᵀW on the lower 128-tiles exactly as nlml_grad_impl forms it (N³/3 flop), mirrored into the upper tiles: the full
    // product would read the tiles of WT below the diagonal, which nothing defines, and cost twice the flop.  A fresh fit's padding
    // rows N … Np are the identity the factorisation left there, so B is finite throughout and D's zero padding removes them from T
    GemmArgs a{};
    a.A = g->st->WT.as<double>(); a.lda = ld; a.B = g->st->WT.as<double>(); a.ldb = ld;
    a.C = g->T.as<double>(); a.ldc = Np; a.M = (int)Np; a.N = (int)Np; a.K = (int)Np;
    a.kmode = K_A_UPPER; a.lower_only = 1; a.batch = 1; a.alpha = 1.0; a.beta = 0.0;
    HIPCHK(launch_gemm_nt(a, s));
    HIPCHK(launch_loo_mirror(g->T.as<double>(), Np, (int)Np, s));
    // D = ∂K/∂log ℓ, T = B·D (D symmetric: the NT product is the product wanted)
    HIPCHK(launch_dkdlogell(g->st->Xs.as<double>(), N, (int)Np, g->dp, g->prm.family, g->prm.sigma_f2, g->Kxz.as<double>(), Np, s));
    GemmArgs b{};
    b.A = g->T.as<double>(); b.lda = Np; b.B = g->Kxz.as<double>(); b.ldb = Np;
    b.C = g->loo_T.as<double>(); b.ldc = Np; b.M = (int)Np; b.N = (int)Np; b.K = (int)Np;
    b.kmode = K_FULL; b.lower_only = 0; b.batch = 1; b.alpha = 1.0; b.beta = 0.0;
    HIPCHK(launch_gemm_nt(b, s));
    LooGradArgs ga{};
    ga.T = g->loo_T.as<double>(); ga.B = g->T.as<double>(); ga.alpha = g->alpha.as<double>(); ga.partial = g->partial.as<double>();
    ga.out = ga.partial + 3 * (size_t)nb; ga.ld = Np; ga.N = N; ga.noise = g->st->noise_used;
    HIPCHK(launch_loo_grad_rows(ga, s));
    double o[3];
    HIPCHK(hipMemcpyAsync(o, ga.out, sizeof o, hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    if (d_log_ell) *d_log_ell = o[0];
    if (d_log_sigma_f2) *d_log_sigma_f2 = o[1];
    if (d_log_noise) *d_log_noise = ga.noise == 0.0 ? 0.0 : o[2];
    return ABO_OK;
}

}  // extern "C"

constexpr int64_t COV_MAX_POINTS = 8192;          // points per set of abo_predict_cov and abo_acq_kg

namespace {

// what abo_predict_cov and abo_acq_kg check alike, before any device work; *Mb becomes Ma in the symmetric form
int32_t cov_check(abo_gp* g, const char* fn, const double* Za, int64_t Ma, const double* Zb, int64_t* Mb, int32_t d, int32_t z_space,
                  int32_t out_space) {
    if (!g) return fail(ABO_EINVAL, "%s: null handle", fn);
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    if (g->p_out > 1)
        return fail(ABO_EINVAL, "%s: a gradient-enhanced model has p outputs per point (abo_predict_grad_cov gives the block of one point)", fn);
    if (d != g->d) return fail(ABO_EDIM, "DimensionMismatch: %s with d = %d, model dimension %d", fn, d, g->d);
    if ((z_space != ABO_HOST && z_space != ABO_DEVICE) || (out_space != ABO_HOST && out_space != ABO_DEVICE))
        return fail(ABO_EINVAL, "%s: z_space %d / out_space %d is neither ABO_HOST nor ABO_DEVICE", fn, z_space, out_space);
    if (Ma < 1 || Ma > COV_MAX_POINTS) return fail(ABO_EINVAL, "%s: Ma = %lld outside 1..%lld", fn, (long long)Ma, (long long)COV_MAX_POINTS);
    if (!Za) return fail(ABO_EINVAL, "%s: Za is NULL", fn);
    if (!Zb) {
        if (*Mb != 0 && *Mb != Ma)
            return fail(ABO_EINVAL, "%s: Zb is NULL (the symmetric form), Mb = %lld is neither 0 nor Ma = %lld", fn, (long long)*Mb, (long long)Ma);
        *Mb = Ma;
    } else if (*Mb < 1 || *Mb > COV_MAX_POINTS) {
        return fail(ABO_EINVAL, "%s: Mb = %lld outside 1..%lld", fn, (long long)*Mb, (long long)COV_MAX_POINTS);
    }
    return ABO_OK;
}

// The V and product stage both calls share.  Per set: K_ZX from the generator (the mean falls out of the same pass: abo_predict's bits),
// V = K_ZX·L⁻ᵀ on the fp64 GEMM against the lower-triangular W (k ≤ i: half the product), its columns ≥ N zeroed — rows ≥ N of shared
// factor storage may hold a discarded appended branch, and a 128-tile of W reaches past the view's N.  Then the prior block (cov.hip) and
// the product subtracted in place (C = −V_a·V_bᵀ + C).  Zb == NULL: the lower 128-tiles only, mirrored.  Launches only, on the handle's
// stream; every workspace of the stage is sized before its first launch (pack: doubles of Kxz the caller wants behind it).
struct CovBlock {
    bool sym;
    int64_t Map, Mbp;
    double* V[2];          // V_a, V_b (= V_a in the symmetric form): [Mp][Np]
    double* mu[2];         // the means of the two sets (mu[1] = mu[0] in the symmetric form)
    double* C;             // [Map][Mbp], zero padded
};
int32_t cov_block(abo_gp* g, const double* Za, int64_t Ma, const double* Zb, int64_t Mb, int32_t z_space, bool want_cov,
                  const bool want_set[2], size_t pack, CovBlock* out) {
    hipStream_t s = g->stream;
    const int64_t Np = g->Np, ld = g->st->cap;
    const int N = (int)g->N, dp = g->dp, d = g->d;
    const bool sym = Zb == nullptr;
    const int64_t Map = pad_up(Ma, TB), Mbp = pad_up(Mb, TB);
    const int nsets = sym ? 1 : 2;
    const int64_t Ms[2] = {Ma, Mb}, Mps[2] = {Map, Mbp};
    const double* Zin[2] = {Za, Zb};
    // every workspace before the first launch: a buffer that grew between two launches would go back to the pool with work queued on it
    if (z_space == ABO_HOST) HIPCHK(g->Zdev.ensure(sizeof(double) * (size_t)(Ma + (sym ? 0 : Mb)) * d));
    HIPCHK(g->mu_all.ensure(sizeof(double) * (size_t)(Map + Mbp)));
    if (want_cov) {
        const size_t kx = (size_t)(Map > Mbp ? Map : Mbp) * Np;                                          // K_ZX of one set, later the compact block
        HIPCHK(g->Kxz.ensure(sizeof(double) * (kx > pack ? kx : pack)));
        HIPCHK(g->cov_Zs.ensure(sizeof(double) * (size_t)(Map + (sym ? 0 : Mbp)) * dp));
        HIPCHK(g->cov_V.ensure(sizeof(double) * (size_t)(Map + (sym ? 0 : Mbp)) * Np));
        HIPCHK(g->cov_C.ensure(sizeof(double) * (size_t)Map * Mbp));
    }
    double* Vset[2] = {g->cov_V.as<double>(), g->cov_V.as<double>() + (want_cov ? Map * Np : 0)};
    double* Zsset[2] = {g->cov_Zs.as<double>(), g->cov_Zs.as<double>() + (want_cov ? Map * dp : 0)};
    double* muset[2] = {g->mu_all.as<double>(), g->mu_all.as<double>() + Map};
    for (int q = 0; q < nsets; ++q) {
        if (!want_cov && !want_set[q]) continue;
        const double* Zd = Zin[q];
        if (z_space == ABO_HOST) {
            double* stage = g->Zdev.as<double>() + (q ? Ma * d : 0);
            HIPCHK(hipMemcpyAsync(stage, Zin[q], sizeof(double) * (size_t)Ms[q] * d, hipMemcpyHostToDevice, s));
            Zd = stage;
        }
        KgenArgs ka = kgen_model_args(g, true);             // (one output: pt = 1, and mean_vec is its [0] alone)
        ka.Z = Zd; ka.alpha = g->alpha.as<double>(); ka.Kout = want_cov ? g->Kxz.as<double>() : nullptr;
        ka.mu = muset[q]; ka.ldk = Np; ka.M = Ms[q]; ka.Mc = (int)Mps[q];
        HIPCHK(launch_kgen(ka, s));
        if (!want_cov) continue;
        HIPCHK(launch_scale_points(Zd, Zsset[q], (int)Ms[q], (int)Mps[q], g->d, dp, 1.0 / g->prm.ell, s));
        GemmArgs a{};               // V[j][i] = Σ_{k ≤ i} Kzx[j][k]·W[i][k] = (L⁻¹k(X, z_j))[i]; padded rows j ≥ M are zero as those of Kzx are
        a.A = g->Kxz.as<double>(); a.lda = Np; a.B = g->st->W.as<double>(); a.ldb = ld;
        a.C = Vset[q]; a.ldc = Np; a.M = (int)Mps[q]; a.N = (int)Np; a.K = (int)Np;
        a.kmode = K_B_LOWER; a.batch = 1; a.alpha = 1.0; a.beta = 0.0;
        HIPCHK(launch_gemm_nt(a, s));
        HIPCHK(launch_qei_zero_tail(Vset[q], Np, N, (int)Np, (int)Mps[q], s));
    }
    double* Cp = want_cov ? g->cov_C.as<double>() : nullptr;
    if (want_cov) {
        HIPCHK(launch_cov_prior(Zsset[0], Zsset[sym ? 0 : 1], (int)Ma, (int)Mb, dp, g->prm.family, g->prm.sigma_f2, sym ? 1 : 0, Cp, Mbp, s));
        GemmArgs b{};               // C −= V_a·V_bᵀ
        b.A = Vset[0]; b.lda = Np; b.B = Vset[sym ? 0 : 1]; b.ldb = Np; b.C = Cp; b.ldc = Mbp;
        b.M = (int)Map; b.N = (int)Mbp; b.K = (int)Np; b.kmode = K_FULL; b.lower_only = sym ? 1 : 0; b.batch = 1; b.alpha = -1.0; b.beta = 1.0;
        HIPCHK(launch_gemm_nt(b, s));
        if (sym) HIPCHK(launch_loo_mirror(Cp, Mbp, (int)Map, s));
    }
    *out = CovBlock{sym, Map, Mbp, {Vset[0], Vset[sym ? 0 : 1]}, {muset[0], muset[sym ? 0 : 1]}, Cp};
    return ABO_OK;
}

}  // namespace

extern "C" {

// Joint posterior covariance between two point sets (include/abo_hip.h): the shared stage above, then the compact copy-out.  Always the
// fp64 engine: the int8-residue contraction squares one operand, a signed cross product is outside its error analysis.
int32_t abo_predict_cov(abo_gp* g, const double* Za, int64_t Ma, const double* Zb, int64_t Mb, int32_t d, int32_t z_space, double* mu_a,
                        double* mu_b, double* cov, int32_t out_space) {
    if (const int32_t rc = cov_check(g, "abo_predict_cov", Za, Ma, Zb, &Mb, d, z_space, out_space)) return rc;
    const bool sym = Zb == nullptr;
    if (sym && mu_b) return fail(ABO_EINVAL, "abo_predict_cov: Zb is NULL (the symmetric form) but mu_b is given; the means are mu_a");
    if (!mu_a && !mu_b && !cov) return ABO_OK;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const bool host_out = out_space == ABO_HOST;
    const bool want_set[2] = {mu_a != nullptr, mu_b != nullptr};
    CovBlock cb{};
    if (const int32_t rc = cov_block(g, Za, Ma, Zb, Mb, z_space, cov != nullptr, want_set, cov && host_out ? (size_t)Ma * Mb : 0, &cb)) return rc;
    if (cov) {
        double* packed = host_out ? g->Kxz.as<double>() : cov;
        HIPCHK(launch_cov_pack(cb.C, cb.Mbp, (int)Ma, (int)Mb, sym ? 1 : 0, packed, s));
        if (host_out) HIPCHK(hipMemcpyAsync(cov, packed, sizeof(double) * (size_t)Ma * Mb, hipMemcpyDeviceToHost, s));
    }
    double* const mu_out[2] = {mu_a, mu_b};
    const int64_t Ms[2] = {Ma, Mb};
    for (int q = 0; q < (sym ? 1 : 2); ++q) {
        if (!mu_out[q]) continue;
        const int32_t rc = copy_out(mu_out[q], cb.mu[q], sizeof(double) * (size_t)Ms[q], out_space, s);
        if (rc) return rc;
    }
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

// Knowledge gradient over a discrete decision set (include/abo_hip.h): the covariance stage of abo_predict_cov, then per
// candidate the variance and the slope scale (kg.hip: launch_kg_prep), the row kernel on the padded block where it lies, and the
// library's selection on the scores.  Nothing of the Ma × Mb block goes to the host.
int32_t abo_acq_kg(abo_gp* g, const double* Za, int64_t Ma, const double* Zb, int64_t Mb, int32_t d, int32_t z_space, double noise,
                   int32_t flags, int64_t idx_base, double* scores, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space) {
    if (const int32_t rc = cov_check(g, "abo_acq_kg", Za, Ma, Zb, &Mb, d, z_space, out_space)) return rc;
    const bool sym = Zb == nullptr;
    if (flags & ~ABO_KG_SELF) return fail(ABO_EINVAL, "abo_acq_kg: flags = %d holds bits other than ABO_KG_SELF", flags);
    if (sym && (flags & ABO_KG_SELF))
        return fail(ABO_EINVAL, "abo_acq_kg: ABO_KG_SELF with Zb NULL (the symmetric form holds every candidate's own point already)");
    if (!std::isfinite(noise)) return fail(ABO_EINVAL, "abo_acq_kg: noise is not finite (negative: the noise the factor was built with)");
    if (k < 0) return fail(ABO_EINVAL, "abo_acq_kg: k = %d is negative", k);
    if (k > 0 && (!top_val || !top_idx)) return fail(ABO_EINVAL, "abo_acq_kg: k > 0 needs top_val and top_idx");
    if (idx_base < 0) return fail(ABO_EINVAL, "abo_acq_kg: idx_base = %lld is negative", (long long)idx_base);
    if (!scores && k == 0) return ABO_OK;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const bool host_out = out_space == ABO_HOST;
    const double nz = noise < 0.0 ? g->st->noise_used : noise;
    // this call's own workspaces, like the stage's before the first launch
    HIPCHK(g->kg_w.ensure(sizeof(double) * 2 * (size_t)Ma));
    double* sc_d = scores;
    if (!scores || host_out) { HIPCHK(g->score_all.ensure(sizeof(double) * (size_t)Ma)); sc_d = g->score_all.as<double>(); }
    TopkWork w{};
    double* tv = top_val;
    int64_t* ti = top_idx;
    if (k > 0) {
        const int64_t we = topk_workspace_entries(Ma, k);
        HIPCHK(g->tk_keys0.ensure(sizeof(uint64_t) * we));
        HIPCHK(g->tk_keys1.ensure(sizeof(uint64_t) * we));
        HIPCHK(g->tk_idx0.ensure(sizeof(int64_t) * we));
        HIPCHK(g->tk_idx1.ensure(sizeof(int64_t) * we));
        w = TopkWork{{g->tk_keys0.as<uint64_t>(), g->tk_keys1.as<uint64_t>()}, {g->tk_idx0.as<int64_t>(), g->tk_idx1.as<int64_t>()}};
        if (host_out) {
            HIPCHK(g->top_val.ensure(sizeof(double) * k));
            HIPCHK(g->top_idx.ensure(sizeof(int64_t) * k));
            tv = g->top_val.as<double>();
            ti = g->top_idx.as<int64_t>();
        }
    }
    const bool want_set[2] = {true, true};
    CovBlock cb{};
    if (const int32_t rc = cov_block(g, Za, Ma, Zb, Mb, z_space, true, want_set, 0, &cb)) return rc;
    double* den = g->kg_w.as<double>();
    double* self_b = den + Ma;
    // v_i: the symmetric form's diagonal; the rectangular form's from the squared row norms of V_a (one wave per row, launch_kg_prep)
    HIPCHK(launch_kg_prep(cb.V[0], g->Np, (int)g->N, sym ? cb.C : nullptr, cb.Mbp, (int)Ma, g->prm.sigma_f2, nz, den, self_b, s));
    KgArgs ka{};
    ka.a = cb.mu[1]; ka.asign = -1.0; ka.B = cb.C; ka.ldb = cb.Mbp; ka.den = den;
    if (flags & ABO_KG_SELF) { ka.self_a = cb.mu[0]; ka.self_b = self_b; }
    ka.Ma = (int)Ma; ka.Mb = (int)Mb; ka.val = sc_d; ka.nenv = nullptr;
    HIPCHK(launch_kg_rows(ka, s));
    if (k > 0) {
        HIPCHK(launch_topk(sc_d, Ma, k, idx_base, w, tv, ti, s));
        if (host_out) {
            if (const int32_t rc = copy_out(top_val, tv, sizeof(double) * k, ABO_HOST, s)) return rc;
            if (const int32_t rc = copy_out(top_idx, ti, sizeof(int64_t) * k, ABO_HOST, s)) return rc;
        }
    }
    if (scores && host_out)
        if (const int32_t rc = copy_out(scores, sc_d, sizeof(double) * (size_t)Ma, ABO_HOST, s)) return rc;
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

// host vector of a gradient-enhanced model: the library's point-major order v[i·p + q] → the ABI's by-outputs order v[q·N + i]
static void to_by_outputs(double* v, int64_t N, int p) {
    std::vector<double> t(v, v + N * p);
    for (int64_t i = 0; i < N; ++i)
        for (int q = 0; q < p; ++q) v[(int64_t)q * N + i] = t[i * p + q];
}

int32_t abo_get_n(abo_gp* g, int64_t* N, int32_t* d) {
    if (!g) return fail(ABO_EINVAL, "null handle");
    if (N) *N = g->fitted ? g->npts : 0;
    if (d) *d = g->fitted ? g->d : 0;
    return ABO_OK;
}

int32_t abo_get_prune_stats(abo_gp* g, abo_prune_stats* out) {
    if (!g || !out) return fail(ABO_EINVAL, "abo_get_prune_stats: null argument");
    *out = g->pst;
    return ABO_OK;
}

int32_t abo_get_prune_levels(abo_gp* g, int64_t* out) {
    if (!g || !out) return fail(ABO_EINVAL, "abo_get_prune_levels: null argument");
    out[0] = g->plv.rows1; out[1] = g->plv.s1; out[2] = g->plv.rows2; out[3] = g->plv.s2;
    out[4] = (int64_t)llround(g->plv.ms1 * 1e3); out[5] = (int64_t)llround(g->plv.ms2 * 1e3);      // whole microseconds
    return ABO_OK;
}

int32_t abo_get_timings(abo_gp* g, abo_timings* out) {
    if (!g || !out) return fail(ABO_EINVAL, "abo_get_timings: null argument");
    *out = g->tm;
    return ABO_OK;
}

int32_t abo_get_factor(abo_gp* g, double* L, double* alpha, double* Linv) {
    if (!g) return fail(ABO_EINVAL, "null handle");
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    HIPCHK(hipSetDevice(g->prm.device));
    const int64_t N = g->N;
    hipStream_t s = g->stream;
    if (L) {
        HIPCHK(hipMemcpy2DAsync(L, sizeof(double) * N, g->st->K.p, sizeof(double) * g->st->cap, sizeof(double) * N, N,
                                hipMemcpyDeviceToHost, s));
    }
    if (Linv) {
        HIPCHK(hipMemcpy2DAsync(Linv, sizeof(double) * N, g->st->W.p, sizeof(double) * g->st->cap, sizeof(double) * N, N,
                                hipMemcpyDeviceToHost, s));
    }
    if (alpha) HIPCHK(hipMemcpyAsync(alpha, g->alpha.p, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    if (alpha && g->p_out > 1) to_by_outputs(alpha, g->npts, g->p_out);
    if (L)   // off-diagonal upper blocks of the in-place factor still hold K: present a clean L
        for (int64_t i = 0; i < N; ++i)
            for (int64_t j = i + 1; j < N; ++j) L[i * N + j] = 0.0;
    return ABO_OK;
}

int32_t abo_get_data(abo_gp* g, double* X, double* y) {
    if (!g) return fail(ABO_EINVAL, "null handle");
    if (!g->fitted) return fail(ABO_EINVAL, "surrogate is not conditioned on data yet (call abo_fit first)");
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    if (X) HIPCHK(hipMemcpyAsync(X, g->st->Xraw.p, sizeof(double) * g->npts * g->d, hipMemcpyDeviceToHost, s));
    if (y) HIPCHK(hipMemcpyAsync(y, g->st->ybuf.p, sizeof(double) * g->N, hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    if (y && g->p_out > 1) to_by_outputs(y, g->npts, g->p_out);
    return ABO_OK;
}

}  // extern "C"

// ---- optimize_acquisition on the device (acq_utils.jl:33-73): refinement launch + the one-call driver -----------------
namespace abo {    // shared with test_hooks.hip (abo_state.h)
RefineOpts refine_defaults(const abo_refine_opts* o) {
    RefineOpts r{100, 20, 10, 1e-5, 2.2e-9, 1e-4};        // acq_utils.jl:10, :62; Optim's LBFGS keeps m = 10 pairs
    if (o) {
        // clamped: "no limit" spelled as INT32_MAX must not overflow the round budget max_iter × linesearch_max (refine.hip) nor
        // size the curvature-pair storage
        if (o->max_iter > 0) r.max_iter = o->max_iter < 10000 ? o->max_iter : 10000;
        if (o->linesearch_max > 0) r.ls_max = o->linesearch_max < 64 ? o->linesearch_max : 64;
        if (o->history > 0) r.history = o->history < 64 ? o->history : 64;
        if (o->g_tol > 0.0) r.g_tol = o->g_tol;
        if (o->f_abstol > 0.0) r.f_abstol = o->f_abstol;
        if (o->x_abstol > 0.0) r.x_abstol = o->x_abstol;
    }
    return r;
}

int32_t check_refinable(abo_gp* g, int32_t d, const char* fn) {
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (g->p_out > 1 && d + 1 != g->p_out) return fail(ABO_EINVAL, "%s: gradient-enhanced handle with p = %d outputs and d = %d", fn, g->p_out, d);
    return ABO_OK;
}
}  // namespace abo

namespace {

hipError_t grad_eval_cb(void* ctx, const double* pts, int npts, double* mu, double* cov, hipStream_t) {
    abo_gp* g = static_cast<abo_gp*>(ctx);
    // (a failure inside is reported through the calling thread's error slot; the launcher only needs "not hipSuccess")
    return grad_eval_device(g, pts, npts, 0.0, mu, cov, nullptr) == ABO_OK ? hipSuccess : hipErrorUnknown;
}

}  // namespace

namespace abo {    // shared with test_hooks.hip (abo_state.h)
// bounds (2·d doubles: lower, upper), starts (S·d) and the outputs all in DEVICE memory; asynchronous on the handle's stream
// between EV_ACQ_BEGIN and EV_ACQ_SCORED (abo_refine*) or the EV_REFINE_* pair (abo_optimize_acquisition*): the caller records them
int32_t refine_device(abo_gp* g, const AcqTerms& terms, const double* bounds_d, const double* starts_d, int S,
                      RefineOpts o, double* x_out_d, double* f_out_d, int* iters_d, int grad_only) {
    hipStream_t s = g->stream;
    RefineArgs ra{};
    ra.Xs = g->st->Xs.as<double>(); ra.W = g->st->W.as<double>(); ra.WT = g->st->WT.as<double>(); ra.alpha = g->alpha.as<double>();
    ra.ld = g->st->cap; ra.N = (int)g->N; ra.Np = (int)g->Np; ra.d = g->d; ra.dp = g->dp; ra.family = g->prm.family;
    ra.s = 1.0 / g->prm.ell; ra.sigma_f2 = g->prm.sigma_f2; ra.mean_c = g->prm.mean_c;
    ra.terms = terms;
    ra.lower = bounds_d; ra.upper = bounds_d ? bounds_d + g->d : nullptr; ra.starts = starts_d;
    ra.x_out = x_out_d; ra.f_out = f_out_d; ra.iters_out = iters_d;
    // the L-BFGS state of a start lives in its workgroup's LDS (64 KiB without opting into more): fewer pairs for very wide inputs
    int m = o.history;
    while (m > 0 && refine_lds_bytes(g->d, g->dp, m) > 65536) --m;
    if (refine_lds_bytes(g->d, g->dp, m) > 65536)
        return fail(ABO_EINVAL, "abo_refine: input dimension %d too large for the on-device refinement (library limit: %d)", g->d, 700);
    ra.max_iter = o.max_iter; ra.ls_max = o.ls_max; ra.history = m; ra.g_tol = o.g_tol; ra.f_abstol = o.f_abstol; ra.x_abstol = o.x_abstol;
    // MES is evaluated by the StandardGP kernels only (refine.hip: objective_value_and_partials<true>); rl_grad_ev_kernel below goes
    // through terms_value_and_partials, which has no case for it
    if (g->p_out > 1 && terms_mes(terms)) return fail(ABO_EINVAL, "abo_refine: max-value entropy search on a gradient-enhanced handle");
    if (g->p_out > 1) {
        // gradient-enhanced model: lockstep rounds over the all-output posterior (refine.hip: launch_refine_lockstep_grad) — value
        // and gradient of the function-value terms come out of ONE mean / covariance-block evaluation per point
        const bool stencil = terms_have_gradnorm(terms);
        const size_t wb = refine_lockstep_grad_bytes(S, g->d, m, stencil);
        HIPCHK(g->T.ensure(wb + sizeof(double) * MAX_P));
        double* mean_g = reinterpret_cast<double*>(static_cast<char*>(g->T.p) + wb);
        HIPCHK(hipMemcpyAsync(mean_g, g->mean_vec + 1, sizeof(double) * g->d, hipMemcpyHostToDevice, s));
        GradEval ev{g, grad_eval_cb};
        const hipError_t e = grad_only ? launch_acq_grad_via_eval(ra, S, mean_g, g->T.p, ev, s)
                                       : launch_refine_lockstep_grad(ra, S, mean_g, g->T.p, ev, s);
        if (e == hipErrorUnknown) return ABO_EHIP;            // grad_eval_device has set the error text
        HIPCHK(e);
        return ABO_OK;
    }
    // from 1024 factor rows on the starts advance in lockstep rounds whose evaluations are batched on the MFMA tile core (L⁻¹ read once
    // per round instead of once per start and evaluation; measured crossover, profiles/r03_optimize_acquisition_latency.txt: N = 500
    // 2.56 ms one launch / 2.96 lockstep, N = 1024 6.98 / 4.16); ABO_REFINE_LOCKSTEP_NP moves the switch (0 = never)
    const char* lke = getenv("ABO_REFINE_LOCKSTEP_NP");
    const long lock_np = lke ? atol(lke) : 1024L;
    if (!grad_only && lock_np > 0 && g->Np >= lock_np) {
        HIPCHK(g->T.ensure(refine_lockstep_bytes(S, (int)g->Np, g->d, m)));
        HIPCHK(launch_refine_lockstep(ra, S, g->T.p, s));
        return ABO_OK;
    }
    HIPCHK(g->T.ensure(sizeof(double) * 4 * (size_t)g->Np * (size_t)S));      // per-start scratch (k, κ', v, u); T is free after the fit
    ra.scratch = g->T.as<double>();
    HIPCHK(launch_refine(ra, S, grad_only, s));
    return ABO_OK;
}
}  // namespace abo

namespace {

// the best refined point, the reference's way (acq_utils.jl:66-72: strict `>` keeps the first maximum); the best grid point if no
// refined value reaches its score
void pick_best(const double* starts_x, const double* starts_val, const double* rx, const double* rf, int k, int d, double* best_x,
               double* best_val) {
    int j = -1;
    for (int e = 0; e < k; ++e) {
        const double v = rf[e];
        if (!(v == v) || std::fabs(v) > 1.0e300) continue;
        if (j < 0 || v > rf[j]) j = e;
    }
    const double* src = starts_x;
    double val = k > 0 ? starts_val[0] : std::numeric_limits<double>::quiet_NaN();
    if (j >= 0 && (rf[j] >= val || !(val == val))) { src = rx + (size_t)j * d; val = rf[j]; }
    if (best_x) for (int c = 0; c < d; ++c) best_x[c] = k > 0 ? src[c] : std::numeric_limits<double>::quiet_NaN();
    if (best_val) *best_val = val;
}

}  // namespace

void abo::pick_best_point(const double* starts_x, const double* starts_val, const double* rx, const double* rf, int k, int d,
                          double* best_x, double* best_val) {
    pick_best(starts_x, starts_val, rx, rf, k, d, best_x, best_val);
}

extern "C" {

static int32_t refine_terms_impl(abo_gp* g, const AcqTerms& terms, const double* lower, const double* upper, int32_t d,
                                 const double* starts, int32_t S, const abo_refine_opts* opts, double* x_out, double* f_out,
                                 int32_t* iters_out) {
    if (S < 0 || (S > 0 && (!starts || !x_out || !f_out)) || !lower || !upper) return fail(ABO_EINVAL, "abo_refine: bad argument");
    for (int c = 0; c < d; ++c)
        if (!(lower[c] <= upper[c])) return fail(ABO_EINVAL, "abo_refine: lower[%d] > upper[%d]", c, c);
    if (S == 0) return ABO_OK;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const size_t nb = 2 * (size_t)d, ns = (size_t)S * d;
    // one staging block: bounds | starts | x_out | f_out | iters
    HIPCHK(g->Zdev.ensure(sizeof(double) * (nb + 2 * ns + S) + sizeof(int) * 2 * S));
    double* base = g->Zdev.as<double>();
    double *bd = base, *sd = base + nb, *xd = sd + ns, *fd = xd + ns;
    int* id = reinterpret_cast<int*>(fd + S);
    HIPCHK(hipMemcpyAsync(bd, lower, sizeof(double) * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(bd + d, upper, sizeof(double) * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(sd, starts, sizeof(double) * ns, hipMemcpyHostToDevice, s));
    HIPCHK(g->events(EV_ACQ_END + 1));
    HIPCHK(hipEventRecord(g->evs()[EV_ACQ_BEGIN], s));
    int32_t rc = refine_device(g, terms, bd, sd, S, refine_defaults(opts), xd, fd, id, 0);
    if (rc) return rc;
    HIPCHK(hipEventRecord(g->evs()[EV_ACQ_SCORED], s));
    std::vector<int> it(2 * (size_t)S);
    PinStage pin(g->ctx);
    HIPCHK(pin.d2h(x_out, xd, sizeof(double) * ns, s));
    HIPCHK(pin.d2h(f_out, fd, sizeof(double) * S, s));
    HIPCHK(pin.d2h(it.data(), id, sizeof(int) * 2 * S, s));
    HIPCHK(wait_stream(s));
    pin.flush();
    g->tm.refine_ms = ev_ms(g->evs()[EV_ACQ_BEGIN], g->evs()[EV_ACQ_SCORED]);
    g->tm.refine_starts = S;
    g->tm.refine_evals = 0;
    for (int e = 0; e < S; ++e) g->tm.refine_evals += it[2 * e + 1];
    if (iters_out) for (int e = 0; e < 2 * S; ++e) iters_out[e] = it[e];
    return ABO_OK;
}

int32_t abo_refine_terms(abo_gp* g, const abo_acq_term* terms, int32_t nterms, const double* lower, const double* upper, int32_t d,
                         const double* starts, int32_t S, const abo_refine_opts* opts, double* x_out, double* f_out, int32_t* iters_out) {
    if (!g) return fail(ABO_EINVAL, "abo_refine_terms: null handle");
    int32_t rc = check_refinable(g, d, "abo_refine_terms");
    if (rc) return rc;
    AcqTerms t{};
    rc = make_terms(g, terms, nterms, &t, "abo_refine_terms");
    if (rc) return rc;
    return refine_terms_impl(g, t, lower, upper, d, starts, S, opts, x_out, f_out, iters_out);
}

int32_t abo_refine(abo_gp* g, int32_t kind, double p0, double best_y, const double* lower, const double* upper, int32_t d,
                   const double* starts, int32_t S, const abo_refine_opts* opts, double* x_out, double* f_out, int32_t* iters_out) {
    if (!g) return fail(ABO_EINVAL, "abo_refine: null handle");
    int32_t rc = check_refinable(g, d, "abo_refine");
    if (rc) return rc;
    const abo_acq_term one{kind, 0, p0, best_y, 1.0};
    AcqTerms t{};
    rc = make_terms(g, &one, 1, &t, "abo_refine");
    if (rc) return rc;
    return refine_terms_impl(g, t, lower, upper, d, starts, S, opts, x_out, f_out, iters_out);
}

}  // extern "C"

// The grid stage on one handle (acq_utils.jl:44-52): n-point Latin hypercube generated on the device (rows j0 … j0+count−1 of it),
// scored under `t`, the k best (score, global index) pairs left in DEVICE memory (tv, ti) and — when sd is given — their
// coordinates gathered to sd [k][d].  bounds_d: device {lower[d], upper[d]}.  grid: scratch of count·d doubles.  Synchronises.
static int32_t grid_stage_device(abo_gp* g, const AcqTerms& t, const double* bounds_d, int d, int64_t n, int64_t j0, int64_t count,
                                 uint64_t seed, int k, double* grid, double* tv, int64_t* ti, double* sd) {
    hipStream_t s = g->stream;
    HIPCHK(launch_lhs(grid, n, d, bounds_d, bounds_d + d, seed, j0, count, s));
    int32_t rc = acq_terms_impl(g, grid, count, d, ABO_DEVICE, t, j0, nullptr, ABO_DEVICE, k, tv, ti, ABO_DEVICE);
    if (rc) return rc;
    if (sd) HIPCHK(launch_gather_points(grid, ti, j0, k, d, sd, s));
    return ABO_OK;
}

static int32_t optimize_terms_impl(abo_gp* g, const AcqTerms& t, const double* lower, const double* upper, int32_t d, int64_t n_grid,
                                   int32_t n_local, uint64_t seed, const abo_refine_opts* opts, double* best_x, double* best_val,
                                   double* starts_x, double* starts_val, double* refined_x, double* refined_val) {
    if (!lower || !upper || !best_x) return fail(ABO_EINVAL, "abo_optimize_acquisition: null argument");
    if (n_grid < 1 || n_local < 1) return fail(ABO_EINVAL, "abo_optimize_acquisition: n_grid and n_local must be positive");
    for (int c = 0; c < d; ++c)
        if (!(lower[c] <= upper[c])) return fail(ABO_EINVAL, "abo_optimize_acquisition: lower[%d] > upper[%d]", c, c);
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const int k = (int)(n_local < n_grid ? n_local : n_grid);
    const size_t nb = 2 * (size_t)d, ns = (size_t)k * d;
    // device block of this call: bounds | starts | refined x | refined f | start scores | start indices | iteration counts
    ScratchBuf blk(g->prm.device, s), grid(g->prm.device, s);
    HIPCHK(blk.b.ensure(sizeof(double) * (nb + 2 * ns + 2 * (size_t)k) + sizeof(int64_t) * k + sizeof(int) * 2 * k));
    HIPCHK(grid.b.ensure(sizeof(double) * (size_t)n_grid * d));
    double* bd = blk.b.as<double>();
    double *sd = bd + nb, *xd = sd + ns, *fd = xd + ns, *tv = fd + k;
    int64_t* ti = reinterpret_cast<int64_t*>(tv + k);
    int* id = reinterpret_cast<int*>(ti + k);
    HIPCHK(hipMemcpyAsync(bd, lower, sizeof(double) * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(bd + d, upper, sizeof(double) * d, hipMemcpyHostToDevice, s));
    // grid stage (acq_utils.jl:44-52): Latin hypercube on the device, fused scores, stable reverse sort's first k
    int32_t rc = grid_stage_device(g, t, bd, d, n_grid, 0, n_grid, seed, k, grid.b.as<double>(), tv, ti, sd);
    if (rc) return rc;
    const double grid_ms = g->tm.acq_total_ms;
    // refinement stage (:55-71): one launch
    HIPCHK(g->events(EV_REFINE_END + 1));
    HIPCHK(hipEventRecord(g->evs()[EV_REFINE_BEGIN], s));
    rc = refine_device(g, t, bd, sd, k, refine_defaults(opts), xd, fd, id, 0);
    if (rc) return rc;
    HIPCHK(hipEventRecord(g->evs()[EV_REFINE_END], s));
    std::vector<double> hs(ns), hv(k), hx(ns), hf(k);
    std::vector<int> it(2 * (size_t)k);
    PinStage pin(g->ctx);
    HIPCHK(pin.d2h(hs.data(), sd, sizeof(double) * ns, s));
    HIPCHK(pin.d2h(hv.data(), tv, sizeof(double) * k, s));
    HIPCHK(pin.d2h(hx.data(), xd, sizeof(double) * ns, s));
    HIPCHK(pin.d2h(hf.data(), fd, sizeof(double) * k, s));
    HIPCHK(pin.d2h(it.data(), id, sizeof(int) * 2 * k, s));
    HIPCHK(wait_stream(s));
    pin.flush();
    g->tm.acq_total_ms = grid_ms;
    g->tm.refine_ms = ev_ms(g->evs()[EV_REFINE_BEGIN], g->evs()[EV_REFINE_END]);
    g->tm.refine_starts = k;
    g->tm.refine_evals = 0;
    for (int e = 0; e < k; ++e) g->tm.refine_evals += it[2 * e + 1];
    pick_best(hs.data(), hv.data(), hx.data(), hf.data(), k, d, best_x, best_val);
    if (starts_x) memcpy(starts_x, hs.data(), sizeof(double) * ns);
    if (starts_val) memcpy(starts_val, hv.data(), sizeof(double) * k);
    if (refined_x) memcpy(refined_x, hx.data(), sizeof(double) * ns);
    if (refined_val) memcpy(refined_val, hf.data(), sizeof(double) * k);
    return ABO_OK;
}

// internal (mgpu.hip): a shard's part of the grid stage with the selection left on the device
int32_t abo::acq_lhs_shard(abo_gp* g, const abo_acq_term* terms, int32_t nterms, int64_t n, int32_t d, const double* lower,
                           const double* upper, uint64_t seed, int64_t j0, int64_t count, int32_t k, double* grid_d, double* tv_d,
                           int64_t* ti_d) {
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    AcqTerms t{};
    rc = make_terms(g, terms, nterms, &t, "abo_mgpu_acq_lhs");
    if (rc) return rc;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    ScratchBuf bnd(g->prm.device, s);
    HIPCHK(bnd.b.ensure(sizeof(double) * 2 * (size_t)d));
    double* bd = bnd.b.as<double>();
    HIPCHK(hipMemcpyAsync(bd, lower, sizeof(double) * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(bd + d, upper, sizeof(double) * d, hipMemcpyHostToDevice, s));
    if (count > 0) HIPCHK(launch_lhs(grid_d, n, d, bd, bd + d, seed, j0, count, s));
    return acq_terms_impl(g, grid_d, count, d, ABO_DEVICE, t, j0, nullptr, ABO_DEVICE, k, tv_d, ti_d, ABO_DEVICE);
}

int32_t abo::refine_terms(abo_gp* g, const abo_acq_term* terms, int32_t nterms, const double* lower, const double* upper, int32_t d,
                          const double* starts, int32_t S, const abo_refine_opts* opts, double* x_out, double* f_out) {
    return abo_refine_terms(g, terms, nterms, lower, upper, d, starts, S, opts, x_out, f_out, nullptr);
}

extern "C" {

int32_t abo_optimize_acquisition_terms(abo_gp* g, const abo_acq_term* terms, int32_t nterms, const double* lower, const double* upper,
                                       int32_t d, int64_t n_grid, int32_t n_local, uint64_t seed, const abo_refine_opts* opts,
                                       double* best_x, double* best_val, double* starts_x, double* starts_val, double* refined_x,
                                       double* refined_val) {
    if (!g) return fail(ABO_EINVAL, "abo_optimize_acquisition_terms: null handle");
    int32_t rc = check_refinable(g, d, "abo_optimize_acquisition_terms");
    if (rc) return rc;
    AcqTerms t{};
    rc = make_terms(g, terms, nterms, &t, "abo_optimize_acquisition_terms");
    if (rc) return rc;
    return optimize_terms_impl(g, t, lower, upper, d, n_grid, n_local, seed, opts, best_x, best_val, starts_x, starts_val, refined_x,
                               refined_val);
}

int32_t abo_optimize_acquisition(abo_gp* g, int32_t kind, double p0, double best_y, const double* lower, const double* upper,
                                 int32_t d, int64_t n_grid, int32_t n_local, uint64_t seed, const abo_refine_opts* opts,
                                 double* best_x, double* best_val, double* starts_x, double* starts_val, double* refined_x,
                                 double* refined_val) {
    const abo_acq_term one{kind, 0, p0, best_y, 1.0};
    return abo_optimize_acquisition_terms(g, &one, 1, lower, upper, d, n_grid, n_local, seed, opts, best_x, best_val, starts_x,
                                          starts_val, refined_x, refined_val);
}

// the grid stage alone on ONE handle: what abo_mgpu_acq_lhs is for a group (the Julia shim's grid_stage on a single-device model)
int32_t abo_acq_lhs(abo_gp* g, int64_t n, int32_t d, const double* lower, const double* upper, uint64_t seed, int32_t kind, double p0,
                    double best_y, int32_t k, double* top_val, int64_t* top_idx, double* top_x) {
    if (!g) return fail(ABO_EINVAL, "abo_acq_lhs: null handle");
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (n < 1 || !lower || !upper) return fail(ABO_EINVAL, "abo_acq_lhs: bad grid");
    if (k < 1 || !top_val || !top_idx) return fail(ABO_EINVAL, "abo_acq_lhs: needs k >= 1, top_val and top_idx");
    const abo_acq_term one{kind, 0, p0, best_y, 1.0};
    AcqTerms t{};
    rc = make_terms(g, &one, 1, &t, "abo_acq_lhs");
    if (rc) return rc;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    ScratchBuf blk(g->prm.device, s), grid(g->prm.device, s);
    const size_t nb = 2 * (size_t)d, ns = (size_t)k * d;
    HIPCHK(blk.b.ensure(sizeof(double) * (nb + ns + (size_t)k) + sizeof(int64_t) * k));
    HIPCHK(grid.b.ensure(sizeof(double) * (size_t)n * d));
    double* bd = blk.b.as<double>();
    double *sd = bd + nb, *tv = sd + ns;
    int64_t* ti = reinterpret_cast<int64_t*>(tv + k);
    HIPCHK(hipMemcpyAsync(bd, lower, sizeof(double) * d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(bd + d, upper, sizeof(double) * d, hipMemcpyHostToDevice, s));
    rc = grid_stage_device(g, t, bd, d, n, 0, n, seed, k, grid.b.as<double>(), tv, ti, top_x ? sd : nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(top_val, tv, sizeof(double) * k, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(top_idx, ti, sizeof(int64_t) * k, hipMemcpyDeviceToHost, s));
    if (top_x) HIPCHK(hipMemcpyAsync(top_x, sd, sizeof(double) * ns, hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    if (top_x) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int e = 0; e < k; ++e)
            if (top_idx[e] < 0) for (int c = 0; c < d; ++c) top_x[(size_t)e * d + c] = nan;
    }
    return ABO_OK;
}

}  // extern "C"

// ---- max-value entropy search (ABO_ACQ_MES): the entry points that carry the samples ---------------------------------------
// The scalar entry points take (kind, p0, best_y); MES takes S samples of the minimum value instead, so it has entry points of its own
// that build the objective's one term (AcqTerms::ystar) and run the same stages: acq_terms_impl (posterior pass + epilogue + the
// selection of abo_acq; never the pruned one: terms_plain is false), refine_terms_impl, optimize_terms_impl.

namespace abo {    // shared with test_hooks.hip (abo_state.h)

// the checks that need no handle: they run first
int32_t mes_check_samples(const double* ystar, int32_t S, int32_t ys_space, const char* fn) {
    if (!ystar) return fail(ABO_EINVAL, "%s: null ystar", fn);
    if (S < 1 || S > MES_MAX_SAMPLES) return fail(ABO_EINVAL, "%s: S = %d samples outside 1..%d", fn, S, MES_MAX_SAMPLES);
    if (ys_space != ABO_HOST && ys_space != ABO_DEVICE) return fail(ABO_EINVAL, "%s: unknown memory space %d", fn, ys_space);
    if (ys_space == ABO_HOST)
        for (int i = 0; i < S; ++i)
            if (!std::isfinite(ystar[i])) return fail(ABO_EINVAL, "%s: ystar[%d] is not finite", fn, i);
    return ABO_OK;
}

int32_t mes_check_handle(abo_gp* g, const char* fn) {
    if (g->p_out > 1) return fail(ABO_EINVAL, "%s: max-value entropy search runs on StandardGP handles only (this one is gradient-enhanced)", fn);
    return ABO_OK;
}

// the objective: host samples are copied to the handle's buffer on its stream (in order before every kernel that reads them), device
// samples are read where they are
int32_t mes_terms(abo_gp* g, const double* ystar, int32_t S, int32_t ys_space, AcqTerms* t) {
    *t = AcqTerms{};
    t->n = 1; t->kind[0] = ACQ_MES; t->w[0] = 1.0; t->n_ystar = S;
    if (ys_space == ABO_DEVICE) { t->ystar = ystar; return ABO_OK; }
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(g->ystar.ensure(sizeof(double) * MES_MAX_SAMPLES));
    HIPCHK(hipMemcpyAsync(g->ystar.p, ystar, sizeof(double) * S, hipMemcpyHostToDevice, g->stream));
    t->ystar = g->ystar.as<double>();
    return ABO_OK;
}

}  // namespace abo

extern "C" {

int32_t abo_score_mes(int32_t device, const double* mu, const double* var, int64_t M, const double* ystar, int32_t S, int32_t ys_space,
                      double* scores) {
    if (M < 0 || (M > 0 && (!mu || !var || !scores))) return fail(ABO_EINVAL, "abo_score_mes: bad argument");
    int32_t rc = mes_check_samples(ystar, S, ys_space, "abo_score_mes");
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    ScratchBuf ys(device, nullptr);
    const double* yd = ystar;
    if (ys_space == ABO_HOST) {
        HIPCHK(ys.b.ensure(sizeof(double) * S));
        HIPCHK(hipMemcpyAsync(ys.b.p, ystar, sizeof(double) * S, hipMemcpyHostToDevice, nullptr));
        yd = ys.b.as<double>();
    }
    HIPCHK(launch_score_mes(mu, var, M, yd, S, scores, nullptr, nullptr, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_refine_mes(abo_gp* g, const double* ystar, int32_t S, const double* lower, const double* upper, int32_t d, const double* starts,
                       int32_t n_starts, const abo_refine_opts* opts, double* x_out, double* f_out, int32_t* iters_out) {
    int32_t rc = mes_check_samples(ystar, S, ABO_HOST, "abo_refine_mes");
    if (rc) return rc;
    if (!g) return fail(ABO_EINVAL, "abo_refine_mes: null handle");
    rc = check_refinable(g, d, "abo_refine_mes");
    if (rc) return rc;
    rc = mes_check_handle(g, "abo_refine_mes");
    if (rc) return rc;
    AcqTerms t;
    rc = mes_terms(g, ystar, S, ABO_HOST, &t);
    if (rc) return rc;
    return refine_terms_impl(g, t, lower, upper, d, starts, n_starts, opts, x_out, f_out, iters_out);
}

int32_t abo_optimize_acquisition_mes(abo_gp* g, const double* ystar, int32_t S, const double* lower, const double* upper, int32_t d,
                                     int64_t n_grid, int32_t n_local, uint64_t seed, const abo_refine_opts* opts, double* best_x,
                                     double* best_val, double* starts_x, double* starts_val, double* refined_x, double* refined_val) {
    int32_t rc = mes_check_samples(ystar, S, ABO_HOST, "abo_optimize_acquisition_mes");
    if (rc) return rc;
    if (!g) return fail(ABO_EINVAL, "abo_optimize_acquisition_mes: null handle");
    rc = check_refinable(g, d, "abo_optimize_acquisition_mes");
    if (rc) return rc;
    rc = mes_check_handle(g, "abo_optimize_acquisition_mes");
    if (rc) return rc;
    AcqTerms t;
    rc = mes_terms(g, ystar, S, ABO_HOST, &t);
    if (rc) return rc;
    return optimize_terms_impl(g, t, lower, upper, d, n_grid, n_local, seed, opts, best_x, best_val, starts_x, starts_val, refined_x,
                               refined_val);
}

}  // extern "C"

bool abo::exiting() { return g_exiting.load(); }
void abo::set_exiting() { g_exiting.store(true); }
void abo::arm_exit_guard() {
    // registered AFTER the first successful device call: atexit handlers run in reverse order of registration, so this one
    // runs before the HIP runtime's own teardown (registered when the runtime initialised)
    if (!g_exit_armed.exchange(true)) std::atexit(exit_hook);
}
void abo::at_exit(void (*f)()) { std::lock_guard<std::mutex> lk(g_exit_mu); g_exit_hooks.push_back(f); }
// only the two codes the runtime reserves for "torn down": hipErrorNotInitialized / hipErrorInvalidContext can be spurious mid-run
// errors of one call, and latching the process-wide flag on those would turn every later destroy into a leak
bool abo::gone(hipError_t e) { return e == hipErrorDeinitialized || e == hipErrorContextIsDestroyed; }

// internal accessors for the multi-device driver (mgpu.hip)
hipStream_t abo::gp_stream(abo_gp* g) { return g->stream; }
int abo::gp_device(const abo_gp* g) { return g->prm.device; }
const abo_params& abo::gp_params(const abo_gp* g) { return g->prm; }
int abo::gp_dim(const abo_gp* g) { return g->fitted ? g->d : 0; }
bool abo::gp_append_view(abo_gp* g, AppendView* o) {
    if (!g->fitted || !g->st || !g->from_append || g->p_out != 1 || !g->vext.p) return false;
    *o = AppendView{g->vext.as<double>(), g->ap_s2, g->ap_serial};
    return true;
}
int32_t abo::set_error(int32_t code, const char* text) { return fail(code, "%s", text); }
const char* abo::last_error_text() { return g_err; }

// internal accessors for abo_update (update.hip)
bool abo::gp_state(abo_gp* g, GpState* o) {
    *o = GpState{};
    o->device = g->prm.device;
    o->p_out = g->p_out;
    o->mean_vec = g->mean_vec;
    o->fitted = g->fitted && g->st != nullptr;
    if (!o->fitted) return false;
    Storage* st = g->st;
    o->d = g->d;
    o->npts = g->npts; o->rows = g->N; o->cap_rows = st->cap; o->max_live = st->max_live();
    o->noise_used = st->noise_used;
    o->storage = st;
    o->Xraw = st->Xraw.as<double>(); o->ybuf = st->ybuf.as<double>();
    return true;
}
int32_t abo::gp_append_into(abo_gp* g, abo_gp* n, const double* x, const double* yv, int64_t* info) {
    n->oz_engine = g->oz_engine; n->oz_nmod = g->oz_nmod;
    return g->p_out > 1 ? append_grad_impl(g, n, x, yv, info) : append_impl(g, n, x, yv[0], info);
}
const void* abo::gp_storage(const abo_gp* g) { return g->fitted ? g->st : nullptr; }
bool abo::gp_factor_view(abo_gp* g, FactorView* o) {
    if (!g->fitted || !g->st) return false;
    Storage* st = g->st;
    *o = FactorView{st->Xs.as<double>(), st->W.as<double>(), st->WT.as<double>(), st->cap, st->dp, st->gen};
    return true;
}
char* abo::gp_pin(abo_gp* g, size_t* bytes) {
    if (!g->ctx || !g->ctx->pin) { *bytes = 0; return nullptr; }
    *bytes = PIN_BYTES - PIN_OUT;                    // [0, PIN_OUT) holds a fit's scalars
    return g->ctx->pin + PIN_OUT;
}
hipError_t abo::stream_wait(hipStream_t s) { return wait_stream(s); }
hipError_t abo::scratch_alloc(int dev, size_t bytes, void** p, size_t* cap) { return pool_alloc(dev, bytes, p, cap); }
void abo::scratch_free(int dev, void* p, size_t cap) { pool_free(dev, p, cap); }

extern "C" {

int32_t abo_pool_trim(int32_t device) {
    if (device < 0 || device > 15) return fail(ABO_EINVAL, "abo_pool_trim: bad device %d", device);
    if (g_exiting.load()) return ABO_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    pool_trim(device);
    return ABO_OK;
}

int32_t abo_fill_distance(int32_t device, const double* X, int64_t N, int32_t d, int32_t x_space, const double* S, int64_t n_samples,
                          int32_t s_space, double* out) {
    if (!X || !S || !out) return fail(ABO_EINVAL, "abo_fill_distance: null argument");
    if (N < 1 || n_samples < 1 || d < 1 || d > 65536) return fail(ABO_EINVAL, "abo_fill_distance: bad sizes");
    if (device < 0 || device > 15) return fail(ABO_EINVAL, "abo_fill_distance: bad device %d", device);
    HIPCHK(hipSetDevice(device));
    ScratchBuf xb(device, nullptr), sb(device, nullptr), ob(device, nullptr);
    const double *Xd = X, *Sd = S;
    if (x_space != ABO_DEVICE) {
        HIPCHK(xb.b.ensure(sizeof(double) * (size_t)N * d));
        HIPCHK(hipMemcpyAsync(xb.b.p, X, sizeof(double) * (size_t)N * d, hipMemcpyHostToDevice, nullptr));
        Xd = xb.b.as<double>();
    }
    if (s_space != ABO_DEVICE) {
        HIPCHK(sb.b.ensure(sizeof(double) * (size_t)n_samples * d));
        HIPCHK(hipMemcpyAsync(sb.b.p, S, sizeof(double) * (size_t)n_samples * d, hipMemcpyHostToDevice, nullptr));
        Sd = sb.b.as<double>();
    }
    HIPCHK(ob.b.ensure(sizeof(double)));
    HIPCHK(launch_fill_distance(Xd, N, d, Sd, n_samples, ob.b.as<double>(), nullptr));
    HIPCHK(hipMemcpyAsync(out, ob.b.p, sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_lhs(int32_t device, int64_t n, int32_t d, const double* lower, const double* upper, uint64_t seed, int64_t j0,
                int64_t count, double* Z_dev) {
    if (!lower || !upper || !Z_dev) return fail(ABO_EINVAL, "abo_lhs: null argument");
    if (n < 1 || d < 1 || d > 65536 || j0 < 0 || count < 0 || j0 + count > n) return fail(ABO_EINVAL, "abo_lhs: bad sizes");
    HIPCHK(hipSetDevice(device));
    ScratchBuf sb(device, nullptr);
    DevBuf& b = sb.b;
    HIPCHK(b.ensure(sizeof(double) * 2 * d));
    HIPCHK(hipMemcpyAsync(b.p, lower, sizeof(double) * d, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(b.as<double>() + d, upper, sizeof(double) * d, hipMemcpyHostToDevice, nullptr));
    HIPCHK(launch_lhs(Z_dev, n, d, b.as<double>(), b.as<double>() + d, seed, j0, count, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_score(int32_t device, const double* mu, const double* var, int64_t M, int32_t kind, double p0, double best_y,
                  double* scores) {
    if (M < 0 || (M > 0 && (!mu || !var || !scores))) return fail(ABO_EINVAL, "abo_score: bad argument");
    if (kind == ABO_ACQ_MES) return fail(ABO_EINVAL, "abo_score: ABO_ACQ_MES takes a vector of samples: use abo_score_mes");
    if (!plain_kind(kind)) return fail(ABO_EINVAL, "abo_score: unknown acquisition kind %d", kind);
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_score(mu, var, scores, M, kind, p0, best_y, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

}  // extern "C"
