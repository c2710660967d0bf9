// Internal C++ interface between the single-device host driver (api.hip, posterior.hip, acq.hip, cand.hip, qei_host.hip) and the units
// that see its handles from outside: mgpu.hip (the multi-device driver), update.hip, paths.hip, qei_mc.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "../../include/abo_hip.h"

namespace abo {

// abo_acq / abo_cand_acq with separate memory spaces for the M scores and for the k selected (score, index) pairs
int32_t acq_ex(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, int32_t kind, double p0, double best_y,
               int64_t idx_base, double* scores, int32_t scores_space, int32_t k, double* top_val, int64_t* top_idx,
               int32_t top_space);
int32_t cand_acq_ex(abo_gp* g, abo_cand* c, int32_t kind, double p0, double best_y, int64_t idx_base, double* scores,
                    int32_t scores_space, int32_t k, double* top_val, int64_t* top_idx, int32_t top_space);

int32_t acq_terms_ex(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, const abo_acq_term* terms, int32_t nterms,
                     int64_t idx_base, double* scores, int32_t scores_space, int32_t k, double* top_val, int64_t* top_idx,
                     int32_t top_space);
// a shard's part of the grid stage (acq_utils.jl:44-52): rows j0 … j0+count−1 of the n-point Latin hypercube generated into grid_d
// (device, count·d doubles), scored under the objective, the k best (score, global index) pairs left in tv_d / ti_d (device)
int32_t acq_lhs_shard(abo_gp* g, const abo_acq_term* terms, int32_t nterms, int64_t n, int32_t d, const double* lower,
                      const double* upper, uint64_t seed, int64_t j0, int64_t count, int32_t k, double* grid_d, double* tv_d,
                      int64_t* ti_d);
int32_t refine_terms(abo_gp* g, const abo_acq_term* terms, int32_t nterms, const double* lower, const double* upper, int32_t d,
                     const double* starts, int32_t S, const abo_refine_opts* opts, double* x_out, double* f_out);

// optimize_acquisition's last step on the host (acq_utils.jl:66-72): the refined point with the largest finite value (first on
// ties), or the best grid point when no refined value reaches its score
void pick_best_point(const double* starts_x, const double* starts_val, const double* rx, const double* rf, int k, int d,
                     double* best_x, double* best_val);

// ---- greedy q-EI, block form (qei_host.hip; include/abo_hip.h: abo_cand_qei_*): the per-shard steps with records in DEVICE memory, and
// the batch driver over the n shards of one set (n = 1: abo_cand_qei; n > 1: abo_mgpu_cand_qei, whose shards run on their worker
// threads and exchange records through the group's all-gather)
int32_t qei_eligible(abo_gp* g, abo_cand* c, int q);       // ABO_OK when the block form can run on this shard (else the reason)
int32_t qei_begin(abo_gp* g, abo_cand* c, int q, int T, bool snapshot = true);
int32_t qei_top(abo_gp* g, abo_cand* c, double xi, double best_y, int64_t idx_base, int k, double* rec_d);
int32_t qei_block(abo_gp* g, abo_cand* c, const double* pts, const int64_t* gidx, int T);
int32_t qei_has(const abo_cand* c, int64_t gidx);
int32_t qei_pick(abo_gp* g, abo_cand* c, int64_t gidx, double var_x, const double* cx, int n, int64_t excl, int64_t* info);
int32_t qei_end(abo_gp* g, abo_cand* c);
void qei_get_stats(const abo_cand* c, int picks, double total_ms, abo_qei_stats* out);
struct QeiShards {
    int n;
    abo_gp* const* gp;
    abo_cand* const* cd;
    const int64_t* lo;                                               // global index of each shard's first candidate
    std::function<int32_t(const std::function<int32_t(int)>&)> run;  // f(i) on every shard
    std::function<double*(int)> rec;                                 // shard i's record block (device)
    std::function<int32_t(size_t, double*)> gather;                  // (words, out): every shard's block → host, n × words doubles
};
int qei_block_default();                                            // the process default block size (0: the plain loop)
size_t qei_max_words(int d, int q, int T);                           // doubles a record block must hold
int32_t qei_drive(const QeiShards& S, int q, double xi, double best_y, int distinct, int T, double* x_out, int64_t* idx_out,
                  double* ei_out, int64_t* info);

// ---- Monte-Carlo joint q-EI (qei_mc.hip: abo_cand_qei_mc) on the block state of ONE set.  _open: qei_eligible, then the set's blocks
// continue (or start afresh) as under qei_begin, with the chain left exactly as it is (only its real entries [0, nreal) are read);
// *keep receives the statistics of the set's last greedy batch, which _close puts back.  qei_block builds blocks on the open state.
struct QeiBatchStats { int builds; double block_ms, pass_ms, pass_bytes, pass_flop; };   // block builds of a batch, their time, the last pass over K_ZX
struct QeiMcView {
    double* mu; double* var; const double* Z;        // device, [M], [M], [M][d]
    const double* blk; const double* chain;          // device, [slots][Mp] block columns, [rows][Mp] the set's chain
    int64_t M, Mp;
    int d, T16, nslots, nreal;
    const int* blk_base;                             // host, [nslots / T16]
    const int64_t* slot_gidx;                        // host, [nslots]
    const double* chain_s;                           // host, [nreal …] pivots of the chain entries
    QeiBatchStats now;                              // statistics of the open batch so far
};
// (hidden: the shipped library exports the C-ABI's abo_cand_qei_mc, not these)
__attribute__((visibility("hidden"))) int32_t qei_mc_open(abo_gp* g, abo_cand* c, int q, int T, int64_t idx_base, QeiBatchStats* keep);
__attribute__((visibility("hidden"))) void qei_mc_view(abo_cand* c, QeiMcView* v);        // valid until the next block build
__attribute__((visibility("hidden"))) void qei_mc_close(abo_cand* c, const QeiBatchStats& keep);

hipStream_t gp_stream(abo_gp* g);
int gp_device(const abo_gp* g);
const abo_params& gp_params(const abo_gp* g);
int gp_dim(const abo_gp* g);
const double* cand_points(const abo_cand* c);      // device, [M][d]
const double* cand_mu(const abo_cand* c);          // device, [M]
int64_t cand_size(const abo_cand* c);
int cand_dim(const abo_cand* c);
int cand_device(const abo_cand* c);
// ---- what the advancing sample paths (paths.hip: abo_paths_append) read of an appended model and of a down-dated set
struct CandSync { uint64_t gen; int64_t N; uint64_t mu_epoch; };   // the factor (id, rows) the set is in sync with; mu_epoch grows
void cand_sync(const abo_cand* c, CandSync* out);                  // whenever the set's exclusions may have changed
// the bordered append that made g (false: g is not a one-row abo_append of a standard GP): vext = [−u; 1; 0 …] with
// u = K̃⁻¹k(X, x*) (device, ≥ N entries), s2 = the pivot l_nn², serial = process-wide id of that append
struct AppendView { const double* vext; double s2; uint64_t serial; };
bool gp_append_view(abo_gp* g, AppendView* out);
// the down-date column c(z) over the set, which must be in sync with g: *route 0 = left in place by abo_cand_downdate's pass,
// 1 = the set's chain entry, 2 = recomputed into tmp (device, pad_up(M, 16) doubles)
int32_t cand_downdate_column(abo_gp* g, abo_cand* c, double* tmp, const double** col, int* route);

// ---- abo_update / abo_mgpu_update (update.hip): what they read of a handle, and the append / pool / wait machinery of api.hip
// (the gp_* accessors are api.hip's, the cand_* ones cand.hip's)
struct GpState {
    bool fitted = false;
    int device = 0, d = 0, p_out = 1;
    int64_t npts = 0, rows = 0;          // training points, factor rows (p_out per point)
    int64_t cap_rows = 0;                // capacity of the factor storage, rows
    int64_t max_live = 0;                // rows of the largest live view on that storage (> rows: another view appended past this one)
    double noise_used = 0.0;             // the noise the factor was built with (> noise_var: the jitter ladder ran)
    const void* storage = nullptr;       // identity of the factor storage
    const double* Xraw = nullptr;        // device, [npts][d] as the caller handed them over
    const double* ybuf = nullptr;        // device, [rows] raw targets, point-major (i·p + q)
    const double* mean_vec = nullptr;    // host, p_out prior means
};
bool gp_state(abo_gp* g, GpState* out);   // false: not fitted (device, p_out and mean_vec are filled in all the same)
// the bordered append of one observation (p_out values in yv) to view g, into the fresh handle n (append_impl / append_grad_impl:
// a full refit with doubled capacity when the storage is full or claimed by a larger view)
int32_t gp_append_into(abo_gp* g, abo_gp* n, const double* x, const double* yv, int64_t* info);
const void* gp_storage(const abo_gp* g);
// what the sample paths (paths.hip) read of a fitted model's factor: scaled points [≥ rows][dp], L⁻¹ (lower) and its transpose with
// leading dimension ld, and the process-wide id of the factor storage (never reused, unlike its address)
struct FactorView { const double* Xs; const double* W; const double* WT; int64_t ld; int dp; uint64_t gen; };
bool gp_factor_view(abo_gp* g, FactorView* out);   // false: not fitted
char* gp_pin(abo_gp* g, size_t* bytes);   // the handle's page-locked staging block past the fit scalars (null if it has none)
hipError_t stream_wait(hipStream_t s);     // the polled wait every call ends with
hipError_t scratch_alloc(int dev, size_t bytes, void** p, size_t* cap);   // the device-memory pool
void scratch_free(int dev, void* p, size_t cap);

// Process teardown.  `exiting()` turns true when the process has started to exit (an atexit hook registered behind the HIP
// runtime's own, so it runs BEFORE the runtime tears down, and the library's static destructor): from then on no entry point
// touches the device — a finaliser that runs late (a Julia / Python handle destroyed from an exit handler, a static
// destructor of the host) must find abo_destroy / abo_cand_destroy / abo_mgpu_destroy / pool frees as quiet no-ops, never a
// call into a runtime that is already gone.  `arm_exit_guard()` registers the hook (idempotent; called once a device exists);
// `at_exit(f)` adds work to it (the multi-device driver parks and joins its idle worker threads there).
bool exiting();
void arm_exit_guard();
void at_exit(void (*f)());
// hipSuccess, or an error that only says "the runtime is shutting down" (hipErrorDeinitialized / hipErrorContextIsDestroyed …)
bool gone(hipError_t e);

// the calling thread's last-error slot (abo_last_error reads it)
int32_t set_error(int32_t code, const char* text);
const char* last_error_text();

}  // namespace abo
