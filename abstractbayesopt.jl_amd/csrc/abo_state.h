// Private state of the single-device host driver: what its units — api.hip, posterior.hip, acq.hip, cand.hip, qei_host.hip, and
// test_hooks.hip in the test library — share: the handle and candidate-set structs with the types they are made of, the event slots of
// a handle, and the internal functions that are called across a unit boundary or by the abo_test_* hooks.  Nothing else includes this header: mgpu.hip, update.hip, paths.hip and
// qei_mc.hip see the handles through the accessors of abo_internal.h.  Declarations only: every variable and every function declared
// here is defined once, in the unit its comment names.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <set>
#include <vector>

#include "../../include/abo_hip.h"
#include "abo_internal.h"
#include "abo_kernels.h"

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                    \
    } while (0)
// an event INSIDE a call (api.hip: phase_events says when these are recorded at all)
#define PHASE_EVENT(ev, s) do { if (phase_events()) HIPCHK(hipEventRecord((ev), (s))); } while (0)

struct abo_gp;
struct abo_cand;

#pragma GCC visibility push(hidden)
namespace abo {

int32_t fail(int32_t code, const char* fmt, ...);          // writes the calling thread's slot (abo_last_error), returns code
hipError_t wait_stream(hipStream_t s);                     // the polled wait every call ends with
extern std::atomic<uint64_t> g_storage_gen;                // next Storage::gen
hipError_t pool_alloc(int dev, size_t bytes, void** p, size_t* cap);
void pool_free(int dev, void* p, size_t cap);
// api.hip — what every entry point of the host units starts and ends with
int32_t check_fitted(abo_gp* g, int32_t d);                // also tells phase_events() the size of the model the calling thread works on
int32_t stage_candidates(abo_gp* g, const double* Z, int64_t M, int32_t z_space, const double** Zd);
int32_t copy_in(void* dst, const void* src, size_t bytes, int32_t space, hipStream_t s);
int32_t copy_out(void* dst, const void* src, size_t bytes, int32_t space, hipStream_t s);
bool phase_events();                                       // one definition, one thread-local behind it: a second copy would time N ≤ 128
float ev_ms(hipEvent_t a, hipEvent_t b);                   // 0 for an event that was never recorded
void oz_defaults(int* engine, int* nmod);                  // the process default of the contraction engine (ABO_CONTRACTION, abo_set_contraction)

// Event slots of a handle (abo_gp::evs()).  The numbers are fixed: abo_timings, abo_prune_stats and abo_get_prune_levels are differences
// of these.  EV_REFINE_* ALIASES the W-planes pair: the grid-and-refine call (api.hip: optimize_terms_impl) brackets its refinement
// stage with them, and on a gradient-enhanced handle whose planes of W are stale that stage reaches refine_device → grad_eval_device →
// oz_planes_of_w, which records both again in between — refine_ms then starts at the rebuild.  Kept as it is; not to be copied.
enum EvSlot : size_t {
    EV_FIT_BEGIN = 0, EV_FIT_KMAT = 1, EV_FIT_CHOL = 2, EV_FIT_INV = 3, EV_FIT_END = 4,       // the fit's phases end at 1 … 4
    EV_ACQ_BEGIN = 5, EV_ACQ_SCORED = 6, EV_ACQ_END = 7,                                       // a posterior / acquisition call; a call without selection ends at SCORED
    EV_WPLANES_BEGIN = 8, EV_WPLANES_END = 9,                                                  // residue planes of W rebuilt (posterior.hip: oz_planes_of_w)
    EV_REFINE_BEGIN = EV_WPLANES_BEGIN, EV_REFINE_END = EV_WPLANES_END,                        // alias, see above
    EV_BOUND_BEGIN = 10, EV_BOUND_END = 11, EV_THRESHOLD_END = 12, EV_SURVIVORS_END = 13,      // the pruned selection (acq.hip: prune_select)
    EV_BOUND2_BEGIN = 14, EV_BOUND2_END = 15,                                                  // its second bound level
    // from here on: the per-chunk events of a call's posterior passes (ev_chunk) — or, in calls that run none, scratch: append_impl
    // EV_BASE + 0 … 1, nlml_grad_impl + 0 … 2, qei_block + 0 … 3 (the factorisation's look-ahead kept its strip events here)
    EV_BASE = 16
};
enum EvChunk : size_t {
    EVC_KGEN_BEGIN = 0, EVC_KGEN_END = 1, EVC_CONTRACT_BEGIN = 2, EVC_CONTRACT_END = 3, EVC_EPILOGUE_BEGIN = 4, EVC_EPILOGUE_END = 5,
    EVC_OZ_QUANT_END = 6, EVC_OZ_GEMM_END = 7,          // int8 pipeline, between CONTRACT_BEGIN and CONTRACT_END
    EV_PER_CHUNK = 8
};
// slot of chunk `chunk` of the call (PostPass::chunk0 + c: the passes of one call count on)
inline size_t ev_chunk(int64_t chunk, EvChunk slot) { return (size_t)EV_BASE + (size_t)EV_PER_CHUNK * (size_t)chunk + slot; }

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int dev = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }            // every early return (HIPCHK) hands its buffers back to the pool
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
        return pool_alloc(dev, bytes, &p, &cap);
    }
    void release() { if (p) pool_free(dev, p, cap); p = nullptr; cap = 0; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
#define ABO_DEVBUF_MEMBER(name) abo::DevBuf name;

// stream + events of a handle, recycled the same way (hipStreamCreate / ~400 hipEventCreate per step otherwise)
// pin: a small page-locked host block that lives with the context.  A device-to-host copy of a few bytes into PAGEABLE memory blocks
// the host until it has happened (12 – 14 µs each on this runtime, tools/memcpy_probe.hip; 2.5 – 3.7 µs and asynchronous into
// pinned memory) — four of them were a quarter of a BO step at the reference's own sizes.  The fit's scalars and the selected
// (score, index) pairs land here and are copied on by the host after the call's one synchronisation.
constexpr size_t PIN_BYTES = 32768, PIN_OUT = 64;      // [0,16) fit scalars, [16,24) info, [PIN_OUT, …) selected pairs
struct ExecCtx {
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;
    char* pin = nullptr;
};

// the small read-backs of ONE call: each goes into the context's pinned block (asynchronously) while it fits, straight to its
// destination otherwise; flush() — behind the call's stream synchronisation — copies the staged ones on
struct PinStage {
    ExecCtx* c;
    size_t off = PIN_OUT;
    struct Item { void* dst; size_t off, n; } it[8];
    int n = 0;
    explicit PinStage(ExecCtx* ctx) : c(ctx) {}
    hipError_t d2h(void* dst, const void* src, size_t bytes, hipStream_t s) {
        if (bytes == 0) return hipSuccess;
        const size_t a = (bytes + 15) & ~(size_t)15;
        if (c && c->pin && n < 8 && off + a <= PIN_BYTES) {
            it[n++] = Item{dst, off, bytes};
            const hipError_t e = hipMemcpyAsync(c->pin + off, src, bytes, hipMemcpyDeviceToHost, s);
            off += a;
            return e;
        }
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
    }
    void flush() {
        for (int i = 0; i < n; ++i) memcpy(it[i].dst, c->pin + it[i].off, it[i].n);
        n = 0;
    }
};

constexpr int OZ_DEFAULT_NMOD = 14;   // moduli of the contraction's residue plan unless asked otherwise; P ≈ 2^110: the fixed-point images keep 50+ bits of W per row and 52–53 bits of K_XZ

// a local scratch buffer of one call: on every exit path the stream is drained before the block goes back to the pool
// (an error return must not hand memory that queued work still touches to the next handle)
struct ScratchBuf {
    DevBuf b;
    hipStream_t s;
    ScratchBuf(int dev, hipStream_t st) : s(st) { b.dev = dev; }
    ~ScratchBuf() { if (b.p) { (void)wait_stream(s); b.release(); } }
};

// Heavy device state, shared by every view (copy / appended model) that descends from one fit.
// Rows < N of Xs / delta / L / W / WT are immutable for every live view of size N; an append only
// writes row N of the largest live view, so older views stay valid and rollback is free.
#define ABO_STORAGE_BUFS(X) X(Xraw) X(Xs) X(ybuf) X(delta) X(K) X(W) X(WT)
struct Storage {
    std::atomic<int> refs{1};
    // process-wide unique id: what a candidate set remembers of the factor it is synced with (a freed Storage's address
    // is readily reused by the next refit of the same size; its id never is)
    const uint64_t gen = g_storage_gen.fetch_add(1);
    int dev = 0;
    int d = 0, dp = 0;
    int64_t cap = 0;        // padded capacity = leading dimension of K/W/WT (multiple of 128)
    double noise_used = 0.0;
    // sizes N of the live views on this storage.  A view may append in place only if no live view
    // is larger (rows ≥ its N are then dead: stale rows of discarded fantasy branches are masked
    // everywhere by the view's own N, and the append overwrites row N).
    std::mutex mu;
    std::multiset<int64_t> live;
    void add_view(int64_t n) { std::lock_guard<std::mutex> lk(mu); live.insert(n); }
    void drop_view(int64_t n) { std::lock_guard<std::mutex> lk(mu); auto it = live.find(n); if (it != live.end()) live.erase(it); }
    int64_t max_live() { std::lock_guard<std::mutex> lk(mu); return live.empty() ? 0 : *live.rbegin(); }
    // An append in place writes rows [n_old, n_new): allowed only while no live view reaches beyond n_old — decided AND claimed
    // (the new view registered) under one lock, so that two host threads appending to copies of one model cannot both take the
    // rows (the loser refits into storage of its own: copy-on-write).  A failed append gives the claim back (drop_view).
    bool claim_rows(int64_t n_old, int64_t n_new) {
        std::lock_guard<std::mutex> lk(mu);
        if (!live.empty() && *live.rbegin() > n_old) return false;
        live.insert(n_new);
        return true;
    }
    ABO_STORAGE_BUFS(ABO_DEVBUF_MEMBER)
    void set_device(int dv) {
        dev = dv;
#define X(name) name.dev = dv;
        ABO_STORAGE_BUFS(X)
#undef X
    }
    void release_all() {
#define X(name) name.release();
        ABO_STORAGE_BUFS(X)
#undef X
    }
};
inline void storage_unref(Storage* st) {
    if (st && st->refs.fetch_sub(1) == 1) { st->release_all(); delete st; }
}

}  // namespace abo
#pragma GCC visibility pop

// Every device buffer of a handle, named ONCE: the members, set_device() and free_all() all come from this list.
//   alpha … scal                 the fit: α, the bordered append's vext and work vectors, the workspace T, status word, scalars
//   Zdev … top_idx               posterior workspace: staged candidates, K_XZ chunk, partial sums, μ chunk, full-length arrays, top-k scratch
//   oz_WR … oz_badc              int8-residue contraction (ozaki.hip): residue planes of this view's W (valid for oz_gen / oz_N /
//                                oz_plan.n), row scales and flags, and the per-chunk scratch
//   pr_ub … pr_ti                pruned selection: bounds, gathered points, their scores, survivor list, scan scratch, threshold pairs
//   pr_mut, pr_eps, pr_nrm       its bound pass: μ̃ and ε of every candidate, the norms ε is built from (kgen_tail.hip)
//   pr_ub2, pr_mut2, pr_eps2     second bound level: bounds, μ̃ and ε of the first level's survivors, in list order
//   ystar                        the samples of an abo_*_mes call that came from host memory
//   oz_WRb … oz_delta            the bound pass's short residue plan (ozaki.hip: "the guarded bound"): the residue planes of the first
//                                bound rows of W under it, their row scales, flags and guards — rebuilt by every bound pass
//   loo_T                        abo_loo_grad: T = K̃⁻¹·∂K/∂log ℓ (K̃⁻¹ itself sits in T, ∂K/∂log ℓ in Kxz)
//   cov_Zs, cov_V, cov_C         abo_predict_cov: the scaled points of both sets, V_a / V_b = K_ZX·L⁻ᵀ, the padded covariance block
//   pr_head … pr_hdl             the fused first-level head (kgen_head32.hip): head of μ̃ and S̃ of every candidate, fp32 fragments of
//                                W's head, δ and ‖W_i‖₁
//   pr_ti0                       the K0 candidates of the threshold pass, in the order of their exact scores in pr_sc (pr_ti is
//                                overwritten by the threshold's own selection)
//   pr_xf                        the fp32 tail's training points in fp32, pair-interleaved (kgen_tail32.hip) — written by every bound pass
//                                that reads it
//   kg_w                         abo_acq_kg: sqrt(v_i + noise) and the slope of the own line, per candidate
#define ABO_GP_BUFS(X)                                                                                                              \
    X(alpha) X(vext) X(tvec) X(T) X(info) X(scal)                                                                                   \
    X(Zdev) X(Kxz) X(partial) X(mu_c) X(mu_all) X(var_all) X(score_all) X(tk_keys0) X(tk_keys1) X(tk_idx0) X(tk_idx1) X(top_val) X(top_idx) \
    X(oz_WR) X(oz_sexp) X(oz_badr) X(oz_KR) X(oz_U) X(oz_badc)                                                                      \
    X(pr_ub) X(pr_z) X(pr_sc) X(pr_sel) X(pr_blk) X(pr_tv) X(pr_ti)                                                                 \
    X(pr_mut) X(pr_eps) X(pr_nrm) X(pr_ub2) X(pr_mut2) X(pr_eps2)                                                                   \
    X(ystar) X(oz_WRb) X(oz_sexpb) X(oz_badrb) X(oz_delta) X(loo_T) X(cov_Zs) X(cov_V) X(cov_C)                                     \
    X(pr_head) X(pr_ssq) X(pr_wf) X(pr_hdl) X(pr_ti0) X(pr_xf) X(kg_w)

struct abo_gp {
    std::atomic<int> refs{1};
    abo_params prm{};
    abo::ExecCtx* ctx = nullptr;
    hipStream_t stream = nullptr;      // == ctx->stream
    abo::Storage* st = nullptr;        // null until conditioned on data
    bool fitted = false;
    int64_t N = 0, Np = 0;             // this view's number of factor rows and its 128-padded size
    int64_t npts = 0;                  // training points (== N unless gradient-enhanced: N = p_out·npts)
    int d = 0, dp = 0;
    int p_out = 1;                     // outputs per point: 1 = StandardGP, d+1 = GradientGP (f + gradient)
    double mean_vec[abo::MAX_P] = {0}; // prior mean per output (gradConstMean; [0] = mean_c for p_out == 1)
    double logdet = 0.0, quad = 0.0;
    // bordered-append bookkeeping (valid when this view was produced by abo_append)
    bool from_append = false;
    double ap_s2 = 0.0, ap_beta = 0.0; // Schur complement l_nn² and (y* − μ(x*))/l_nn²
    uint64_t ap_serial = 0;            // process-wide id of the append that made this view (never reused): what a down-date column is tagged with
    std::vector<double> ap_x;          // the point a one-row append added, as the host handed it over (abo_cand_downdate matches it against the q-EI chain)
    double ap_s2v[abo::MAX_P] = {0}, ap_betav[abo::MAX_P] = {0};   // gradient-enhanced append: the same per appended row (p_out of them)
    ABO_GP_BUFS(ABO_DEVBUF_MEMBER)
    // host landing zone of the fit's scalars ({log det, δᵀα} and the LAPACK-style info): read back by one asynchronous copy at
    // the end of the fit's launches and looked at after the NEXT stream synchronisation — the fit's own (abo_fit) or, for
    // abo_fit_acq, the one behind the acquisition launches that were queued right behind the fit
    double h_sc_[2] = {0.0, 0.0};      // (fallback landing zone when the context has no pinned block)
    int64_t h_info_ = 0;
    double* h_sc() { return ctx && ctx->pin ? reinterpret_cast<double*>(ctx->pin) : h_sc_; }
    int64_t& h_info() { return ctx && ctx->pin ? *reinterpret_cast<int64_t*>(ctx->pin + 16) : h_info_; }
    bool fit_small_path = false;
    const double* in_x = nullptr;      // the caller's device arrays while a one-launch fit reads them itself (abo_fit: no staging copies);
    const double* in_y = nullptr;      // null: the model's own copies
    // int8-residue contraction (ozaki.hip): engine choice and the plan the cached planes of W belong to
    int oz_engine = ABO_CONTRACT_AUTO, oz_nmod = 0;
    int* oz_ctr_clean = nullptr;       // the tile-counter block of oz_badc known to hold zeros (OzVarArgs::ctr_clean)
    abo::OzPlan oz_plan{};
    bool oz_prepare_pending = false;  // EV_WPLANES_BEGIN / _END of the current call bracket a rebuild of the residue planes of W (read with its timings)
    uint64_t oz_gen = 0;
    int64_t oz_N = -1;
    // the posterior passes of the current call, in launch order (their per-chunk events are read back with them): the pruned top-k
    // selection of abo_acq runs up to five (two bound levels, threshold, survivors or the fallback's full pass), everything else one
    struct PostPass { int64_t chunk0, nchunk, M, rows; int nmod; bool head32 = false; };   // first chunk's event slot, chunks, candidate rows, rows of W contracted, moduli launched
                                                                                       // (nchunk = 0: nothing was launched — the survivors whose scores came from the threshold pass, counted in the work figures alone)
                                                                                       // (0 and head32: the fused fp32 head of a first bound level, one launch, timed in its first chunk's contraction slot)
    std::vector<PostPass> passes;
    int ph_rows = 0;                                           // rows of the last fused head (0: the last bound pass ran none)
    bool pr_reused = false;                                    // the last abo_acq took its survivors' scores from its threshold pass (abo_test_prune_reused)
    abo_prune_stats pst{};
    struct PruneLevels { int64_t rows1, s1, rows2, s2; double ms1, ms2; } plv{};      // abo_get_prune_levels
    abo::OzPlan oz_plan_b{};                                   // the bound pass's short residue plan
    int pb_rows = 0, pb_sK = 0;                                // rows the last bound pass rebuilt under it, and its scale of K
    abo_timings tm{};

    std::vector<hipEvent_t>& evs() { return ctx->ev; }
    int64_t ld() const { return st->cap; }

    void set_device(int dev) {
#define X(name) name.dev = dev;
        ABO_GP_BUFS(X)
#undef X
    }
    __attribute__((visibility("hidden"))) void free_all();      // api.hip: buffers to the pool, the view off its storage, the context to the free list
    hipError_t events(size_t n) {
        while (ctx->ev.size() < n) {
            hipEvent_t e;
            hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) return r;
            ctx->ev.push_back(e);
        }
        return hipSuccess;
    }
};

// candidate set resident in HBM with its posterior (C5: O(N·M) down-dates instead of re-evaluation) — cand.hip; its block-form
// q-EI state (Qei) is driven by qei_host.hip.  Each device buffer named once, as on the handle.
#define ABO_CAND_BUFS(X)                                                                                                            \
    X(Z) X(mu) X(var) X(score) X(cdot) X(tk_keys0) X(tk_keys1) X(tk_idx0) X(tk_idx1) X(top_val) X(top_idx) X(mu_bak) X(var_bak)      \
    X(Kzx) X(qblk) X(qchain) X(qwork) X(qrec) X(qmu) X(qvar) X(qdev)
struct abo_cand {
    int device = 0, d = 0;
    int64_t M = 0;
    uint64_t synced_gen = 0;              // Storage::gen of the factor the mu/var belong to (0 = none)
    int64_t synced_N = -1;
    uint64_t bak_gen = 0;                 // abo_cand_save snapshot
    int64_t bak_N = -1;
    // the last one-row abo_cand_downdate: the append it served (abo_gp::ap_serial) and where it left the column c(z) — 0: cdot (which
    // nothing else writes), 1: entry dd_chain of the chain.  The resident sample-path values (paths.hip) read the column there.
    uint64_t dd_serial = 0;
    int dd_src = -1, dd_chain = -1;
    uint64_t mu_epoch = 1;                // grows whenever the stored μ — and with it the exclusions — may have changed other than by a down-date
    ABO_CAND_BUFS(ABO_DEVBUF_MEMBER)
    // Kzx: resident K_ZX (candidate-major, kzx_ld doubles per candidate, column k = training row k of synced_st): kept when
    // it fits the budget (ABO_CAND_KZX_GIB, default 64), so that a down-date streams it once instead of re-evaluating
    // N·M kernel values; kzx_ld = 0 → not resident, the down-date recomputes
    int64_t kzx_ld = 0;
    bool resident(const abo_gp* g) const { return kzx_ld > 0 && kzx_ld == g->st->cap; }       // … and laid out for g's factor storage
    bool in_sync(const abo_gp* g) const { return g->st->gen == synced_gen && g->N == synced_N; }
    // block form of greedy q-EI (qei.hip).  Base = the model the set was synced with when the state was last reset (gen, N).
    //   qblk   [nblk_cap][T16][Mp]  covariances Cov(z, x_t) of the block points under the model of the block's build (ring of blocks)
    //   qchain [rows][Mp]           c_i(z) = Cov_{i−1}(z, x_i) of every conditioning since the base, in order: entries [0, nreal) are
    //                               REAL appends (abo_cand_downdate), entries [nreal, nchain) the fantasies of the open / last batch
    // Blocks and real entries OUTLIVE a batch: the next batch on the appended model keeps them (a BO step's picks are mostly the
    // previous step's runners-up: their columns exist already), a block column is corrected by the chain entries made since the
    // block's build (slot_base).  The fantasies of the last batch stay until the next one begins: appending its picks for real, in
    // order, finds each down-date column there (c_i does not depend on the observed value).
    struct Qei {
        bool open = false;
        uint64_t gen = 0;
        int64_t N = -1, Mp = 0;
        int64_t idx_base = -1;                    // the global index of the shard's first candidate the slots below were keyed with (−1: none yet)
        int T16 = 0, nblk_cap = 0, next_blk = 0, qmax = 0;
        std::vector<int64_t> slot_gidx;           // global candidate index per block row (−1: empty)
        std::vector<double> slot_x;               // [rows][d] the block points
        std::vector<int> blk_base;                // [nblk_cap] chain entries that existed when the block was built (already in its columns)
        int nreal = 0, nchain = 0, chain_rows = 0;
        std::vector<double> chain_x;              // [nchain][d] the conditioned points
        std::vector<double> chain_s;              // [nchain] s_i = σ²_{i−1}(x_i) + σ²_n
        abo::QeiBatchStats stats{};               // of the current / last batch
        int batch0 = 0;                           // nchain when the batch began
    } qei;
    void set_device(int dev) {
        device = dev;
#define X(name) name.dev = dev;
        ABO_CAND_BUFS(X)
#undef X
    }
    void free_all() {
#define X(name) name.release();
        ABO_CAND_BUFS(X)
#undef X
        kzx_ld = 0;
        qei = Qei();
    }
};

#pragma GCC visibility push(hidden)
namespace abo {

void set_exiting();                                        // api.hip: latches exiting() — for a destroy that finds the runtime gone
// cand.hip: the k best of the set's M scores sc_d (device), into top_val / top_idx in out_space; launches and copies only
int32_t cand_topk(abo_gp* g, abo_cand* c, const double* sc_d, int32_t k, int64_t idx_base, double* top_val, int64_t* top_idx, int32_t out_space);
int32_t qei_resync(abo_gp* g, abo_cand* c, int64_t rows_now, bool* ok);   // qei_host.hip: the set's block state in line with a model of rows_now rows

// api.hip: the fields of KgenArgs that describe the MODEL of a fitted handle — Xs, N, Np, d, dp, family, s, sigma_f2, pt, and with_mean:
// mean_c, mean_vec (else both zero: the launch forms no mean) —, everything else as KgenArgs{} leaves it.  A call site adds its launch
// (Z, outputs, chunk, layout) and states whatever it wants different of the model.
KgenArgs kgen_model_args(const abo_gp* g, bool with_mean);

// ---- the chunked posterior pass (posterior.hip) ------------------------------------------------------------------------------------------
// what the pass does beyond mu / var / score of M candidates
struct PostOpts {
    int pc = 1;                  // outputs per candidate: 1 = function value; p_out = all outputs of a gradient-enhanced GP (mu / var / score arrays then have pc·M entries)
    bool point_major = false;    // with pc > 1: the rows go point by point (i·pc + q) instead of output by output (q·M + i)
    double* kstore = nullptr;    // write K_XZ into a caller-owned candidate-major matrix (pad_up(M,128) rows of ldstore ≥ Np doubles)
    int64_t ldstore = 0;         // instead of the per-chunk scratch — the resident K_ZX of a candidate set
    // rblocks > 0 (the bound pass of the pruned selection; int8 engine with generator-written planes only, else PRUNE_UNAVAILABLE):
    // the contraction covers the first rblocks 256-row blocks of W — var / score then come from σ²_R ≥ σ² and from μ̃ − ε ≤ μ: the mean's
    // columns past those blocks are summed by the cheaper launch_kgen_tail, which also proves ε ≥ |μ̃ − μ| (kgen_tail.hip).
    int rblocks = 0;
    bool more = false;           // a further pass of the same call — its events and counts are kept next to those of the passes before it
    bool level2 = false;         // a bound pass over the survivors of a first one — μ̃ and ε go to buffers of their own
    bool tail32 = false;         // the tail of a bound pass by launch_kgen_tail32 (fp32 pairs, a wider proven ε: kgen_tail32.hip) — the M-wide first level
    // head32 (with tail32 only): the head of that pass — head of the mean and guarded sum of squares — by ONE launch of kgen_head32.hip over
    // all candidates in place of head generator, residue GEMM and reconstruction per chunk; the chunk loop then runs tail and epilogue alone.
    bool head32 = false;
};
constexpr int32_t PRUNE_UNAVAILABLE = -100;
// mu / var / score for M candidates into device arrays (any may be null); launches only, on the handle's stream
int32_t posterior(abo_gp* g, const double* Zd, int64_t Mpts, int kind, double p0, double best_y, double* mu_out, double* var_out,
                  double* score_out, const PostOpts& o = {});
// gradient-enhanced model: mean of all P outputs, P×P covariance block and GradientNormUCB score per point; launches only
int32_t grad_eval_device(abo_gp* g, const double* Zd, int64_t M, double beta, double* mu_d, double* cov_d, double* sc_d);
// value-only model: the same outputs for the (f, ∇f) posterior, P = d + 1 (abo_predict_deriv); always on the fp64 GEMM; launches only
int32_t deriv_eval_device(abo_gp* g, const double* Zd, int64_t M, double beta, double* mu_d, double* cov_d, double* sc_d);
void collect_posterior_timings(abo_gp* g, bool with_var);  // behind the call's synchronisation: phase times and work of its passes
bool wants_int8(const abo_gp* g, bool want_var, int pc, int* nmod);   // the engine of a posterior call's contraction, and its moduli
double grad_prior_var(const abo_gp* g);                    // prior variance of a gradient output
bool prune_bound_moduli_asked();                           // ABO_PRUNE_BOUND_MODULI is set, or its hook: an explicit request for the int8 head

// ---- scoring and selection (acq.hip) -----------------------------------------------------------------------------------------------------
// scores + selection for host or device candidates, behind check_fitted; separate memory spaces for the M scores and the k selected pairs
int32_t acq_terms_impl(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, const AcqTerms& t, int64_t idx_base,
                       double* scores, int32_t out_space, int32_t k, double* top_val, int64_t* top_idx, int32_t top_space);
int32_t make_terms(const abo_gp* g, const abo_acq_term* terms, int32_t n, AcqTerms* out, const char* fn);
// api.hip: the MES entry points' checks and objective
int32_t mes_check_samples(const double* ystar, int32_t S, int32_t ys_space, const char* fn);
int32_t mes_check_handle(abo_gp* g, const char* fn);
int32_t mes_terms(abo_gp* g, const double* ystar, int32_t S, int32_t ys_space, AcqTerms* t);
// ---- exact top-k without the full variance contraction (DESIGN.md "Pruned top-k selection") -------------------------------------------
// The sum of squares over the first R rows of V = L⁻¹K_XZ is the variance reduction from the first R training points alone, so
// σ²_R = k_zz − Σ_{i<R} V_ij² ≥ σ², and EI, LogEI and UCB (β ≥ 0) do not decrease with σ: the score of (μ, σ²_R) bounds the score from above.
// W = L⁻¹ being triangular, its first R rows cost (R/N)² of the contraction.
struct PrunePlan {
    bool eligible;
    int rblocks;            // 256-row blocks of W in the bound pass
    int64_t k0;             // candidates whose exact scores set the threshold
    int64_t max_survivors;  // more than this: the ordinary full pass runs instead of the survivor pass
    int rblocks0;           // 256-row blocks of a first, narrower bound level over all candidates (0: none — one bound pass, at rblocks)
    int64_t level2_min;     // the pass at rblocks runs on the first level's survivors when there are more than this many
    bool tail32;            // the first level's tail of the mean in fp32 (kgen_tail32.hip); nothing without a first level
    bool head32;            // … and its head — head of the mean, guarded sum of squares — by the fused fp32-MFMA kernel (kgen_head32.hip)
    bool reuse;             // survivors that the threshold pass has scored (S ≤ K0, no second level) are not evaluated again
};
PrunePlan prune_plan(int64_t rows, int64_t M, int k, bool want_scores, int kind, double p0, int p_out, bool int8_fused, int d);
// misc.hip: sc[p] = sc0[q] for the q with idx0[q] == sel[p], p < S = *count (device) — the exact scores of the survivors out of those
// of the threshold pass's K0 candidates; nothing for S > K0; a survivor that is not among the K0 gets NaN and sets *missing (preset to
// 0 by the caller) to 1.  K0 ≤ PRUNE_REUSE_SLOTS / 2.
constexpr int PRUNE_REUSE_SLOTS = 8192;         // ints of LDS (32 KiB): K0 ≤ 4096
hipError_t launch_prune_reuse_scores(const int64_t* sel, const int64_t* count, const int64_t* idx0, const double* sc0, int64_t K0, double* sc,
                                     int64_t* missing, hipStream_t s);
// Overrides of the pruned selection's decisions, "not set" by default and for ever in the shipped library: nothing there writes them, so
// every decision is what the environment and the defaults give.  The abo_test_prune_* hooks (test_hooks.hip) are their only writers.
extern std::atomic<int> g_prune_bound_moduli;       // abo_test_prune_bound_moduli: 0 = the environment's / the default
extern std::atomic<int> g_prune_force_rblocks;      // abo_test_prune_force: row blocks of the bound pass (0 = the rule); mode 1 = a threshold
extern std::atomic<int> g_prune_force_mode;         // of −Inf (every candidate survives: the worst case, on any data), 2 = as ABO_ACQ_PRUNE=0
extern std::atomic<int> g_prune_pre_rblocks;        // abo_test_prune_levels: row blocks of the first level (−1 = none, 0 = the rule)
extern std::atomic<int64_t> g_prune_level2_min;     // … and the survivor count above which the second runs (−1 = the rule)
extern std::atomic<int> g_prune_tail32;             // abo_test_prune_tail32: 0 / 1 = the first level's tail in fp64 / fp32, −1 = the environment's
extern std::atomic<int> g_prune_reuse;              // abo_test_prune_reuse: 0 / 1 = survivors always evaluated / taken from the threshold pass where it holds them, −1 = the environment's
extern std::atomic<int> g_prune_head32;             // abo_test_prune_head32: 0 / 1 = the first level's head on the int8 engine / fused in fp32, −1 = the environment's

// ---- the blocked factorisation on raw pointers (api.hip: factorise runs exactly these two, with the default blocking) -----------------
// SW: columns of a strip, SSmax: of a super-strip, used while at least super_rows rows remain (multiples of 128, SSmax of SW)
struct CholBlocking { int SW = 512, SSmax = 1024, super_rows = 6144; };
// K [Np][ld] → L in place (lower), the 16×16 / 128×128 diagonal inverses in W / WT (rows < Np of both zeroed outside them when
// Np > 128); T: TRSM_STREAM_BYTES of scratch.  Launches only; a failing pivot is reported in *info (device), preset by the caller.
int32_t chol_blocked(double* K, double* W, double* WT, double* T, int64_t ld, int Np, int64_t* info, const CholBlocking& blk, hipStream_t s);
// W = L⁻¹ (lower), WT = its transpose (upper) from the diagonal blocks' inverses, by recursive doubling; T: Np·Np doubles of scratch
int32_t trinv_blocked(double* K, double* W, double* WT, double* T, int64_t ld, int Np, int64_t* info, hipStream_t s);

struct RefineOpts { int max_iter, ls_max, history; double g_tol, f_abstol, x_abstol; };
RefineOpts refine_defaults(const abo_refine_opts* o);
int32_t check_refinable(abo_gp* g, int32_t d, const char* fn);
// bounds (2·d doubles: lower, upper), starts (S·d) and the outputs all in DEVICE memory; asynchronous on the handle's stream
int32_t refine_device(abo_gp* g, const AcqTerms& terms, const double* bounds_d, const double* starts_d, int S, RefineOpts o,
                      double* x_out_d, double* f_out_d, int* iters_d, int grad_only);

}  // namespace abo
#pragma GCC visibility pop
