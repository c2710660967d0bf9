/*
 * abo_hip.h — C-ABI of libabo_hip.so, the MI355X (gfx950) GP-surrogate backend that drops in behind
 * AbstractBayesOpt.jl's AbstractSurrogate / AbstractAcquisition interface.
 *
 * The reference has no FFI of its own (it is pure Julia); each entry point below states the
 * reference function whose arithmetic it replaces (file:line relative to the reference repo) —
 * i.e. what a `HipStandardGP <: AbstractSurrogate` shim would `ccall` from that method
 * (binding shown in INTEGRATION.md).
 *
 * Conventions
 *  - every function returns an int32 status (ABO_OK == 0); on failure abo_last_error() holds text
 *  - points are POINT-MAJOR contiguous fp64: X[i*d + c]  (== a Julia d×N column-major Matrix)
 *  - `*_space` says where a caller buffer lives: ABO_HOST (pageable/pinned host memory) or
 *    ABO_DEVICE (memory of the handle's GPU, e.g. a torch tensor's data_ptr or a hipMalloc)
 *  - calls are synchronous: results are complete (host copies done, device buffers written and
 *    the internal stream idle) when the call returns
 *  - a handle is not re-entrant; different handles may be used from different threads
 *  - indices are 0-based (the Julia shim adds 1)
 */
#ifndef ABO_HIP_H
#define ABO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABO_ABI_VERSION 7   /* 2: abo_mgpu_* (multi-device handles), k and d limits lifted
                               3: abo_set_contraction, abo_timings grew (contraction engine and its phases)
                               4: abo_refine, abo_optimize_acquisition, abo_mgpu_optimize_acquisition, abo_fit_acq, abo_mgpu_create_grad,
                                  abo_mgpu_append_grad; abo_timings grew (refinement stage)
                               5: abo_mgpu_cand_get; abo_acq_lhs (the grid stage on a single handle); weighted-sum objectives and
                                  gradient-enhanced handles in the refinement stage (abo_acq_term, abo_refine_terms,
                                  abo_optimize_acquisition_terms, abo_mgpu_optimize_acquisition_terms, ABO_ACQ_GRADNORM_UCB)
                               6: block form of greedy q-EI: abo_cand_qei (+ _begin / _top / _block / _pick / _end for hosts that
                                  shard the set themselves), abo_qei_stats, abo_set_qei_block, abo_mgpu_cand_qei_stats;
                                  abo_cand_downdate finds the down-date column of a pick appended for real in the batch's chain
                               7: abo_cand_qei_top takes the capacity of the caller's record buffer; abo_cand_qei_eligible (what ranks
                                  that shard a set themselves agree on before they take the block form); abo_cand_qei keeps its
                                  pick loop on the device (one launch per pick, one read-back per batch); abo_fill_distance;
                                  abo_timings grew (abo_nlml_grad phases, the bordered append's mat-vecs); the abo_test_* building
                                  blocks left the shipped library (test build only: ABO_TEST_HOOKS)
                               added within ABI 7 (backwards-compatible, no struct changed): abo_update, abo_mgpu_update,
                                  ABO_UPDATE_SHARED / _APPENDED / _REFIT; abo_cand_qei_mc; abo_paths_create, abo_paths_destroy,
                                  abo_paths_eval, abo_paths_eval_cand, abo_paths_stats_get (struct abo_paths_stats is new); abo_paths_append,
                                  abo_paths_attach, abo_paths_detach, abo_paths_top, abo_paths_values, abo_paths_append_stats_get
                                  (struct abo_paths_append_stats is new); ABO_ACQ_LOGEI (kind 5 in every entry point that takes a kind
                                  or an abo_acq_term, and in the pruned top-k selection); ABO_ACQ_MES and abo_score_mes, abo_acq_mes,
                                  abo_cand_acq_mes, abo_refine_mes, abo_optimize_acquisition_mes; abo_get_prune_levels; abo_loo, abo_loo_grad;
                                  abo_predict_cov; abo_remove, ABO_REMOVE_REMOVED / _REFIT; abo_acq_kg, ABO_KG_SELF; abo_predict_deriv;
                                  abo_append_batch */

/* status codes */
enum {
    ABO_OK = 0,
    ABO_ENOTPD = 1,   /* K + noise·I not positive definite → LinearAlgebra.PosDefException(info)
                         (caught at src/bayesian_opt.jl:126-141) */
    ABO_EDIM = 2,     /* dimension mismatch → DimensionMismatch (test/test_bayesian_opt.jl:788-817) */
    ABO_EINVAL = 3,   /* bad argument / not fitted */
    ABO_EHIP = 4,     /* HIP runtime error */
    ABO_ENOMEM = 5    /* device allocation failed */
};

/* kernel families: k(x,z) = sigma_f2 · kappa(||x−z|| / ell)  (StandardGP normal form,
 * src/surrogates/StandardGP.jl:41-64; kappas: [upstream KernelFunctions] SqExponentialKernel /
 * Matern52Kernel / Matern32Kernel and src/surrogates/GradientGP.jl:94-101, :320-327) */
enum { ABO_KERNEL_SE = 0, ABO_KERNEL_MATERN52 = 1, ABO_KERNEL_MATERN72 = 2, ABO_KERNEL_MATERN32 = 3 };

/* acquisition epilogues */
enum {
    ABO_ACQ_EI = 0,   /* src/acquisition_functions/ExpectedImprovement.jl:40-66   p0 = xi   */
    ABO_ACQ_UCB = 1,  /* src/acquisition_functions/UpperConfidenceBound.jl:38-45  p0 = beta */
    ABO_ACQ_PI = 2,   /* src/acquisition_functions/ProbabilityImprovement.jl:38-63 p0 = xi  */
    ABO_ACQ_MEAN = 3, /* score = −mu (exploitation only; no reference counterpart) */
    ABO_ACQ_GRADNORM_UCB = 4, /* src/acquisition_functions/gradNormUCB.jl:43-51  p0 = beta; gradient-enhanced handles, and only in
                                 the abo_*_terms entry points (abo_predict_grad_cov scores a batch with it directly) */
    ABO_ACQ_LOGEI = 5,/* log EI, p0 = xi and best_y as for EI (no reference counterpart; Ament et al. 2023): log σ + log h(z), h(z) =
                         φ(z) + z·Φ(z), z = Δ/σ, Δ = (best_y − xi) − μ, evaluated so that it is finite for every finite z (EI itself is
                         exactly 0 from z ≈ −39 down, and every such candidate ties); σ² ≤ 1e-12 gives log max(Δ, 0), −Inf for Δ ≤ 0,
                         so that exp(LogEI) = EI on both branches.  Same arg-max and same order as EI wherever EI > 0; standard and
                         gradient-enhanced handles alike (it reads the function output's μ and σ² only).  The q-EI entry points
                         (abo_cand_qei*, abo_cand_qei_mc) keep plain EI. */
    ABO_ACQ_MES = 6   /* max-value entropy search (no reference counterpart; Wang & Jegelka 2017).  Named here for documentation: its
                         parameter is a vector — S samples y*_s of the objective's minimum value — so the entry points that take
                         (kind, p0, best_y) or an abo_acq_term return ABO_EINVAL for it; the abo_*_mes entry points below carry the
                         samples.  MES = (1/S)·Σ_s a(γ_s), γ_s = (μ − y*_s)/σ, a(γ) = γ·φ(γ)/(2Φ(γ)) − log Φ(γ), summed in the order
                         s = 0 … S−1, finite for every finite γ; a ≥ 0 and non-increasing in γ.  σ² ≤ 1e-12 gives 0 (so does a
                         candidate excluded by abo_cand_exclude); a NaN μ or σ² gives NaN.  1 ≤ S ≤ 1024. */
};

/* An objective of the acquisition stage: f(x) = Σ_t weight_t · acq_t(x) on ONE posterior evaluation — EnsembleAcquisition
 * (src/acquisition_functions/EnsembleAcq.jl:12-27, :53-55; the host normalises the weights as the reference's constructor does);
 * a plain acquisition function is one term of weight 1.  At most 8 terms. */
typedef struct abo_acq_term {
    int32_t kind;       /* ABO_ACQ_* */
    int32_t reserved;
    double p0;          /* xi (EI, PI, LOGEI) or beta (UCB, GradientNormUCB) */
    double best_y;      /* EI, PI, LOGEI */
    double weight;
} abo_acq_term;

enum { ABO_HOST = 0, ABO_DEVICE = 1 };

/* engine of the N²·M contraction V = L⁻¹K_XZ behind posterior_var (src/surrogates/StandardGP.jl:377-379):
 *   ABO_CONTRACT_FP64  v_mfma_f64_16x16x4_f64 kernels (78.6 TFLOP/s pipe)
 *   ABO_CONTRACT_INT8  exact products of fixed-point images of the two fp64 operands (K_XZ to 2^-52 of sigma_f2, each row of L⁻¹ to ≥ 50 bits
 *                      below its L1 norm) on v_mfma_i32_16x16x64_i8,
 *                      through residues modulo `nmod` coprime moduli ≤ 256 and a Chinese-remainder reconstruction in fp64
 *                      (14 moduli: errors of the size of the fp64 kernels' own rounding; each modulus less ≈ 14× more error,
 *                      7 % less time).  Serves the posteriors (abo_predict, abo_acq, resident grids; abo_predict_grad and
 *                      abo_predict_grad_cov of a gradient-enhanced handle) up to 65536 factor rows.
 *                      Its scratch is 2·nmod bytes per (candidate, factor row) of a chunk plus nmod·rows² bytes of planes; when the
 *                      device cannot give that (or more than ABO_OZ_SCRATCH_LIMIT_MB allows) the chunk is halved down to 4096
 *                      candidates, and below that the call runs on the fp64 kernels — never an error.
 *   ABO_CONTRACT_AUTO  INT8 from 1280 (padded) factor rows on, FP64 below (the measured crossover: profiles/r06_engine_crossover.txt) */
enum { ABO_CONTRACT_AUTO = 0, ABO_CONTRACT_FP64 = 1, ABO_CONTRACT_INT8 = 2 };

typedef struct abo_gp abo_gp;     /* opaque, reference-counted: one (immutable) conditioned model */
typedef struct abo_cand abo_cand; /* opaque: a candidate set resident in HBM together with its posterior */

typedef struct abo_params {
    int32_t family;     /* ABO_KERNEL_* */
    int32_t device;     /* HIP device ordinal this handle lives on */
    double ell;         /* lengthscale  (get_lengthscale, src/surrogates/StandardGP.jl:261) */
    double sigma_f2;    /* kernel scale (get_scale, :274) */
    double noise_var;   /* observation noise variance (StandardGP.noise_var, :13) */
    double mean_c;      /* prior mean: 0 = ZeroMean, c = ConstMean(c) (:42-44, :223-229) */
    double jitter;      /* 0 = reference behaviour (never add jitter); >0 = opt-in retry with
                           noise_var + jitter·10^r, r = 0..3, when the factorisation fails */
    int64_t n_max;      /* capacity hint for appends (0 = size to the fit) */
    int64_t chunk;      /* candidate chunk size for the posterior (0 = auto) */
} abo_params;

/* phase timings of the last fit / acq call, milliseconds, measured with HIP events on the
 * handle's own stream (see abo_get_timings).  The *_total_ms fields are always measured; the phase fields inside a call
 * (kernel matrix / Cholesky / ..., kxz / var_gemm / finalize / topk, the oz_* fields) are instrumentation: recorded for every
 * model of more than one 128-row block, left out (they read 0) for a one-block model — N <= 128, the reference's own loops,
 * where ~40 event records are a fifth of a 0.2 ms step.  ABO_PHASE_EVENTS=1 records them always, =0 never. */
typedef struct abo_timings {
    double fit_kernel_matrix_ms, fit_cholesky_ms, fit_inverse_ms, fit_alpha_ms, fit_total_ms;
    double acq_kxz_ms, acq_var_gemm_ms, acq_finalize_ms, acq_topk_ms, acq_total_ms;
    int64_t var_gemm_launches;   /* number of launches of the dominant kernel in the last acq */
    double var_gemm_flop;        /* algorithmic flop (N²·M, triangular) those launches performed */
    double downdate_ms;          /* last abo_cand_downdate on this handle: its O(N·M) pass (K_ZX mat-vec or kernel sweep) */
    double downdate_bytes;       /* bytes of resident K_ZX that pass streamed (8·N·M); 0 when it re-evaluated the kernel */
    /* ABI 3: which engine ran the contraction of the last posterior call (ABO_CONTRACT_FP64 / _INT8; 0 = none), and for the
     * int8 engine its moduli count, its phases (acq_var_gemm_ms is their sum: quantisation of K_XZ, residue GEMMs,
     * reconstruction) and the ALGORITHMIC int8 operations of the GEMM launches, moduli × N²·M (one launch per chunk covers all
     * moduli; what the kernel issues beyond the triangular product is not credited).  oz_prepare_ms: residue planes of L⁻¹, spent in
     * the last posterior call (0 when that call reused cached planes) */
    int64_t contraction_engine, oz_nmod;
    double oz_prepare_ms, oz_quant_ms, oz_gemm_ms, oz_crt_ms, oz_gemm_ops;
    /* ABI 4: the last abo_refine / abo_optimize_acquisition on this handle: duration of its ONE refinement launch, the starts it
     * refined and the acquisition evaluations (value + analytic gradient each) all starts took together */
    double refine_ms;
    int64_t refine_starts, refine_evals;
    /* ABI 6: 1 when the last abo_cand_downdate on this handle took its column from the chain of the set's last block-form q-EI
     * batch (no pass over K_ZX: downdate_bytes = 0, downdate_ms = the new K_ZX column only) */
    int64_t downdate_from_chain;
    /* ABI 7: the last abo_nlml_grad on this handle: K⁻¹ = L⁻ᵀL⁻¹ on the fp64 MFMA GEMM (N³/3 flop, lower tiles), and the
     * sweep that generates ∂K/∂log ℓ tile by tile and reduces tr((K⁻¹ − ααᵀ)∂K/∂θ) */
    double nlml_kinv_ms, nlml_trace_ms;
    /* ABI 7: the bordered append that made this handle (abo_append): its two triangular mat-vecs l = L⁻¹k, v = L⁻ᵀl together (HIP
     * events; 0 without phase events) and the bytes they stream, 8·N² (one triangle of L⁻¹ and of L⁻ᵀ, once each) */
    double append_trmv_ms, append_trmv_bytes;
} abo_timings;

/* The pruned top-k selection of the last abo_acq / abo_fit_acq on a handle (abo_get_prune_stats).  A call that asks for the top k
 * only (k > 0, scores == NULL) with EI, LOGEI, or UCB with β ≥ 0, on a StandardGP whose contraction runs on the int8-residue engine, over at
 * least 4·K₀ candidates, does not compute σ² of every candidate: a bound pass over the first bound_rows rows of L⁻¹ gives σ²_R ≥ σ²
 * and so an upper bound of every score; the exact scores of the K₀ = max(4k, 1024) best-by-bound candidates set a threshold; only the
 * candidates whose bound reaches it (the survivors) go through the full contraction.  The k pairs returned are bit for bit those of
 * the full evaluation.  ABO_ACQ_PRUNE=0 in the environment turns the path off.  All zeros: the call was not eligible.
 * From 3072 factor rows on the bound has two levels (abo_get_prune_levels): a first pass over N/32 rows on all candidates sets the
 * threshold, and the pass over N/8 rows runs on its survivors only, when more than 4·K₀ of them are left. */
typedef struct abo_prune_stats {
    int64_t pruned;        /* 1: the k pairs came from the survivor pass */
    int64_t fallback;      /* 1: more than 7/8 of the candidates survived — the ordinary full pass ran behind the passes below */
    int64_t bound_rows;    /* rows of L⁻¹ the bound pass over ALL candidates contracted (0: no bound pass ran) */
    int64_t k0;            /* candidates evaluated exactly for the threshold */
    int64_t survivors;     /* candidates whose bound (of the last level that ran) reached the threshold: what went through the full
                              contraction, or would have without the fallback (the k0 that set the threshold are re-evaluated among them) */
    double bound_ms, threshold_ms, survivor_ms;      /* HIP events on the handle's stream around the passes (bound_ms: every bound pass) */
} abo_prune_stats;

/* --- lifetime -------------------------------------------------------------------------------
 * StandardGP(kernel, noise_var; mean) (src/surrogates/StandardGP.jl:41-64).  The handle starts
 * un-conditioned (gpx === nothing). */
int32_t abo_create(const abo_params* params, abo_gp** out);
/* GradientGP(kernel, p, noise_var; mean=gradConstMean(c)) (src/surrogates/GradientGP.jl:617-639): gradient-
 * enhanced GP with p = d+1 outputs per point (f and ∂f/∂x_c), multi-output kernel gradKernel (:573-606) with
 * analytic derivatives, rows ordered by outputs (MOInputIsotopicByOutputs).  mean_c: p prior means (NULL = 0).
 * 2 ≤ p ≤ 129 (d ≤ 128 inputs; d ≤ 32: the derivative blocks are generated from register-resident coordinates, beyond that from
 * slabs of 32 coordinates, fp64 output only — ABI 7; rounds 2 - 5 stopped at d = 32).
 * abo_fit then takes y of length p·N ordered by outputs (prep_output, :893-895); abo_predict / abo_acq address
 * the function output.  Inside the library the (d+1)N-row system is kept POINT-MAJOR (row i·p + q: all outputs of point i
 * adjacent), so that a new observation appends p rows at the end of the factor (abo_append_grad); every vector that crosses
 * the ABI (y, alpha) is by outputs, abo_get_factor's L / Linv are in the library's row order. */
int32_t abo_create_grad(const abo_params* params, int32_t p, const double* mean_c, abo_gp** out);
/* Engine of the variance contraction for this handle and the models appended from it (gp == NULL: the process default, which
 * new handles start from; the environment variable ABO_CONTRACTION = auto | fp64 | int8 | int8:<nmod> seeds it).  nmod: 8 … 16
 * moduli, 0 = 14.  No reference counterpart: the reference computes this product in fp64 BLAS ([upstream AbstractGPs]
 * diag_Xt_invA_X); both engines meet the same parity bounds (tests/test_gpu_ozaki.py). */
int32_t abo_set_contraction(abo_gp* gp, int32_t engine, int32_t nmod);
/* Base.copy(::StandardGP) (src/surrogates/StandardGP.jl:26, surrogates_utils.jl:12-14): device
 * state is immutable after fit, so a copy is a shared reference. */
int32_t abo_retain(abo_gp* gp);
/* finaliser; frees device state when the last reference goes */
int32_t abo_destroy(abo_gp* gp);

/* --- update ---------------------------------------------------------------------------------
 * update(model::StandardGP, xs, ys) (src/surrogates/StandardGP.jl:79-83): full refit,
 * K = k(X,X) + noise·I, L = chol(K), delta = y − mean_c, alpha = K⁻¹ delta, W = L⁻¹.
 * *info = 0 on success, k>0 (1-based LAPACK potrf convention) with status ABO_ENOTPD when the
 * leading minor of order k is not positive definite; the handle then stays un-conditioned. */
int32_t abo_fit(abo_gp* gp, const double* X, int64_t N, int32_t d, const double* y, int32_t space,
                int64_t* info);

/* update(model, xs, ys) + scores = acqf(model, grid) + sortperm(scores; rev=true)[1:k] — abo_fit followed by abo_acq — in ONE call
 * with ONE host synchronisation: the acquisition's launches are queued directly behind the fit's, the LAPACK-style `info` and the
 * fit's scalars are read once, at the end (after a failed factorisation the acquisition's launches run on leftovers and their
 * results are discarded: status ABO_ENOTPD, *info as abo_fit, outputs untouched in meaning).  What a BO loop at the reference's own
 * sizes (5 … 100 points, 10 000 grid points, acq_utils.jl:37) spends most of its step on is the host round trip between the two
 * calls.  The handle ends up exactly as after abo_fit.  best_y is the caller's (EI / PI take min(ys), ExpectedImprovement.jl:81-83).
 * With an opt-in jitter (abo_params.jitter > 0) or a gradient-enhanced handle the two calls run one after the other. */
int32_t abo_fit_acq(abo_gp* gp, const double* X, int64_t N, int32_t d, const double* y, int32_t space, int64_t* info, const double* Z,
                    int64_t M, int32_t z_space, int32_t kind, double p0, double best_y, int64_t idx_base, double* scores, int32_t k,
                    double* top_val, int64_t* top_idx, int32_t out_space);

/* --- incremental update (BASELINE config 5; no counterpart in the reference, which always refits —
 * nearest code: update(), src/surrogates/StandardGP.jl:79-83) -------------------------------------
 * Bordered ("rank-1 append") Cholesky update: returns in *out a NEW model conditioned on the N+1
 * points that shares the factor storage of `gp`; `gp` itself stays valid and unchanged (rows ≤ N of
 * the factor are never touched), which is what the driver's rollback needs (src/bayesian_opt.jl:116-141).
 *   k = k(X,x), l = L⁻¹k, l_nn² = k(x,x) + noise − ‖l‖² (ABO_ENOTPD, *info = N+1 if ≤ 0),
 *   L' = [[L,0],[lᵀ,l_nn]], α' = [α − βv ; β] with v = K⁻¹k, β = (y − m − kᵀα)/l_nn².
 * O(N²) flops, two passes over L⁻¹.  Falls back to a full refit (with doubled capacity) when the
 * storage is full (abo_params.n_max) or while a LARGER model on the same storage is still alive
 * (destroying the fantasy models of a q-EI exploration makes their parent appendable in place again).
 * x: d host doubles. */
int32_t abo_append(abo_gp* gp, const double* x, int32_t d, double y, int64_t* info, abo_gp** out);
/* the same for a gradient-enhanced model (abo_create_grad): y holds the p observed values {f(x), ∂f/∂x_1 … ∂f/∂x_d}; the
 * p rows are appended one after the other at the end of the point-major factor (each a bordered update whose kernel row
 * comes from the analytic derivative blocks of gradKernel, src/surrogates/GradientGP.jl:573-606), O(p·N²p²) instead of the
 * O(N³p³) refit the reference does per step (update(::GradientGP), :659-668).  params.n_max counts POINTS.  On failure
 * *info is the order of the failing leading minor in the library's row order (N·p + q + 1).  abo_cand_* work on such a
 * handle too (function-value grid; a down-date after abo_append_grad is p rank-1 down-dates). */
int32_t abo_append_grad(abo_gp* gp, const double* x, int32_t d, const double* y, int64_t* info, abo_gp** out);

/* update(model, xs, ys) (src/surrogates/StandardGP.jl:79-83, GradientGP.jl:659-668) that reuses `prev` when (X, y) extends the data
 * prev is conditioned on — what the BO loop passes every iteration (src/bayesian_opt.jl:119-125: the previous points plus the one just
 * evaluated, under standardisation constants fixed before the loop).  The bordered appends run when ALL of these hold:
 *   prev is fitted, d matches, N ≥ Nprev;
 *   X[0:Nprev], y[0:Nprev] equal prev's points and targets bit for bit (checked on the device by one pass over N·(d + p)·8 bytes;
 *     −0.0 against 0.0 or another NaN payload is a mismatch; for a gradient-enhanced handle y is by outputs, as abo_fit takes it);
 *   family, ell, sigma_f2, noise_var, mean_c, jitter (and, for a gradient-enhanced handle, the p values of mean_c) bitwise equal prev's;
 *   prev's factor was built with noise_var itself (a jittered factor goes back through the refit's jitter ladder);
 *   the k = N − Nprev new points make k·p ≤ kmax(R) appended rows, R = prev's factor rows (the crossover rule below);
 *   prev's storage has room for them and no other view appended past prev (else: refit with capacity max(n_max, 2N) points).
 * Then: k bordered appends (abo_append / abo_append_grad semantics, agreeing with the refit to rounding), or for k = 0 a new
 * reference to prev.  Anything else: the same refit abo_create(_grad) + abo_fit would do, with a handle of prev's kind.
 * Crossover rule: kmax(R) = clamp(R / 128, 4, 64) rows.  Measured (profiles/update_latency.txt, k sequential appends against one
 * refit, d = 8, Matérn-5/2): they cost as much as the refit at k ≈ 10 for N = 1024 (rule: 8) and beyond k = 64 for N = 8192 (ratio
 * 0.84 at 64; rule: 64); the floor of 4 rows (one point of a d = 3 gradient-enhanced model) is not measured.
 * `prev` stays valid and unchanged.  *path (may be NULL): ABO_UPDATE_SHARED / _APPENDED / _REFIT = what ran.  space: ABO_HOST /
 * ABO_DEVICE as abo_fit.  A failed append with jitter = 0: ABO_ENOTPD with *info = the order of the failing leading minor, as a
 * refit's potrf reports it (Nprev + j + 1; gradient-enhanced: the library's row order, abo_append_grad); with jitter > 0 the refit
 * runs instead (its jitter ladder applies exactly as in abo_fit).  The intermediate views of a failed sequence are destroyed and give
 * their rows back, so prev stays appendable.  mean_c: p values for a gradient-enhanced prev (NULL = 0), ignored otherwise. */
enum { ABO_UPDATE_SHARED = 0, ABO_UPDATE_APPENDED = 1, ABO_UPDATE_REFIT = 2 };
int32_t abo_update(abo_gp* prev, const abo_params* params, const double* mean_c, const double* X, int64_t N, int32_t d,
                   const double* y, int32_t space, int64_t* info, int32_t* path, abo_gp** out);

/* The model without k of its observations, in O(k·N²): the inverse of abo_append (DESIGN.md "Removing an observation").  idx: k
 * strictly increasing point indices in [0, N) (host array), 1 ≤ k, N − k ≥ 1.  *out is a new handle conditioned on the remaining
 * points in their original order, on factor storage of its own, with gp's parameters, prior mean, the noise gp's factor was built
 * with (a jittered factor stays jittered) and a capacity of n_max points; gp and every other view of its storage stay valid and
 * keep their bits (only rows and columns < N of the storage are read).  Removing row j changes L by a rank-one update of the
 * block behind j whose vector is read off column j of L⁻¹; L⁻¹, α, log det and δᵀα follow in closed form, so no step can fail:
 * there is no ABO_ENOTPD.  One removal streams the triangles of L and L⁻ᵀ once and writes L, L⁻ᵀ and L⁻¹ of the new model.
 * k > 1 runs as k single removals, highest index first.  The new handle counts as freshly fitted for every entry point
 * (abo_append, abo_update as prev, abo_nlml(_grad, _grad_ard), abo_loo(_grad), abo_predict_cov, abo_acq* under both contraction
 * engines, abo_cand_create, abo_paths_create).  Candidate sets and sample paths in sync with gp stay with gp: on the new model a
 * set needs abo_cand_refresh.
 * Crossover rule: k > kmax(N) = clamp(N / 512, 4, 16) gathers the remaining points on the device and refits them
 * (*path = ABO_REMOVE_REFIT: abo_create + abo_fit on that data, bit for bit; a jittered gp goes through the jitter ladder again).
 * Measured (profiles/remove_latency.txt, k single removals against one refit of the rest, d = 8, Matérn-5/2): ratio 0.69 at k = 4 and
 * 1.36 at k = 8 for N = 1024 (rule: 4); 0.47 at k = 8, 0.96 at k = 16 and 1.9 at k = 32 for N = 8192 (rule: 16).  One removal
 * against the refit: 0.10 vs 0.54 ms at N = 1024, 0.74 vs 11.3 ms at N = 8192, 2.49 vs 54.1 ms at N = 16384 (j = 0, the worst
 * case).  The floor of 4 below N = 1024 and the cap of 16 above N = 8192 are not measured.
 * *path (may be NULL): ABO_REMOVE_REMOVED / _REFIT = what ran.  ABO_EINVAL, before any device work: a null, unfitted or
 * gradient-enhanced handle, k < 1, N − k < 1, indices unsorted, repeated or out of range. */
enum { ABO_REMOVE_REMOVED = 0, ABO_REMOVE_REFIT = 1 };
int32_t abo_remove(abo_gp* gp, const int64_t* idx, int32_t k, int32_t* path, abo_gp** out);

/* The model conditioned on k more observations in ONE blocked bordered step: the inverse of abo_remove, and what a batch loop calls
 * after it has evaluated the q points of greedy_qei / mc_qei / thompson_batch in parallel.  X: k × d doubles,
 * row-major; y: k values; both in `space` (ABO_HOST / ABO_DEVICE).  *out is a new view on gp's factor storage, conditioned on gp's
 * N points followed by the k new ones in the given order; gp and every other view stay valid and keep their bits, as with abo_append.
 * With W = L⁻¹, K_b = k(X_train, X_b) (N × k), δ_b = y − mean_c:
 *   B = W·K_b,   S = k(X_b, X_b) + noise_used·I − BᵀB = L_s·L_sᵀ,   C = Wᵀ·B = K⁻¹K_b,
 *   L' = [[L, 0], [Bᵀ, L_s]],   W' = [[W, 0], [−L_s⁻¹Cᵀ, L_s⁻¹]],   r = δ_b − K_bᵀα,  β = S⁻¹r,  α' = [α − Cβ ; β],
 *   logdet' = logdet + 2·Σ log diag L_s,   quad' = quad + ‖L_s⁻¹r‖².
 * The two products stream one triangle of L⁻¹ / L⁻ᵀ each ONCE for all k columns (k sequential abo_append stream them k times and
 * wait for the host k times), as skinny products on the fp64 matrix pipe; one host read-back per step.
 *   k = 1        abo_append's own code path: bit for bit its result, a view abo_cand_downdate / abo_paths_append follow.
 *   2 ≤ k ≤ 64   one blocked step.
 *   k > 64       successive blocked steps of at most 64 rows; the intermediate views are released.
 * A non-positive pivot j (0-based within the batch) of S: ABO_ENOTPD with *info = N + j + 1, the order of the failing leading minor
 * as a refit's potrf reports it; the claimed rows are given back (those of released intermediate views too) and gp stays appendable.
 * No room in the storage, or another view has appended past gp: the N + k points are gathered on the device and refitted with
 * capacity max(n_max, 2(N + k)), exactly as abo_append falls back; abo_timings.append_trmv_bytes of the result then reads 0.
 * The result is an appended view: abo_nlml_grad* refuse it; abo_predict*, abo_acq* under both contraction engines, abo_nlml, abo_loo,
 * abo_predict_cov, abo_acq_kg, abo_remove, abo_append, abo_append_batch and abo_update (as prev) work on it.  For k ≥ 2 a candidate
 * set or sample paths in sync with gp stay with gp: abo_cand_downdate / abo_paths_append on the new view return ABO_EINVAL (the set
 * needs abo_cand_refresh), as after abo_remove.
 * abo_timings of the new handle: append_trmv_ms = the two block products (phase events on), append_trmv_bytes = 8·N² per blocked
 * step.  The same call on the same view gives the same bits every time (no floating-point atomics; the inner dimension of a product
 * is cut into a fixed number of slices that are added in slice order).
 * ABO_EINVAL, before any device work: a null or unfitted handle, a gradient-enhanced handle, k < 1, d not the model's, a null X or y.
 * Measured (profiles/append_batch_latency.txt, d = 8, Matérn-5/2, ms, median):
 *     N = 1024    k = 8: 0.16 (8 sequential abo_append 0.50, refit 0.65)   k = 16: 0.16 (0.99, 0.65)   k = 64: 0.39 (3.88, 0.66)
 *     N = 8192    k = 4: 0.39 (0.53, 12.0)   k = 16: 0.42 (2.28, 12.2)   k = 32: 0.54 (4.84, 12.4)   k = 64: 0.96 (10.2, 12.3)
 *     N = 16384   k = 4: 1.03 (1.50, 57.3)   k = 16: 1.06 (6.40, 58.2)   k = 64: 2.03 (27.8, 58.1)
 * The blocked step is below the sequential appends from k = 4 on and below the refit everywhere in the table (k = 64 at N = 1024:
 * 0.60 of it).  At k = 2 it is SLOWER than the sequential appends (0.39 against 0.26 ms at N = 8192; 1.04 against 0.76 at 16384),
 * at k = 3 level with them (0.40 against 0.40 ms at N = 8192; 0.80 and 0.91 of them at N = 1024 and 16384): its two block products
 * take three times the device time of one append's mat-vec pair (0.26 against 0.087 ms at N = 8192), whatever k up to 16; a caller
 * with two points may as well call abo_append twice.  No crossover rule is applied.
 * Scratch of a step, from the pool and back to it on return: about 11·N·kp doubles, kp = k padded to 16 (92 MB at N = 16384, k = 64). */
int32_t abo_append_batch(abo_gp* gp, const double* X, int32_t k, int32_t d, const double* y, int32_t space, int64_t* info, abo_gp** out);

/* --- posterior ------------------------------------------------------------------------------
 * posterior_mean / posterior_var (src/surrogates/StandardGP.jl:361-363, :377-379), fused as in
 * unstandardized_mean_and_var's mean_and_var (:395-404):
 *   mu = mean_c + K_ZX·alpha,   var = sigma_f2 − colsum((L⁻¹K_XZ)²) + 1e-18  (latent variance).
 * mu / var may each be NULL. */
int32_t abo_predict(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, double* mu,
                    double* var, int32_t out_space);

/* posterior_grad_mean / posterior_grad_var (src/surrogates/GradientGP.jl:936-956): all p outputs of M points,
 * ordered by outputs (p·M values each; mu / var may be NULL). */
int32_t abo_predict_grad(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, double* mu,
                         double* var, int32_t out_space);
/* posterior_grad_cov(model, [x]) per point (GradientGP.jl:966-971): mu [M][p], cov [M][p][p] (point-major) and,
 * if score != NULL, the GradientNormUCB value −(mᵀm + trΣ) + β·sqrt(max(4mᵀΣm + 2‖Σ‖_F², 1e-12)) on the gradient
 * block (src/acquisition_functions/gradNormUCB.jl:43-51).  Any output may be NULL. */
int32_t abo_predict_grad_cov(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, double beta,
                             double* mu, double* cov, double* score, int32_t out_space);

/* added within ABI 7: the same three outputs for a VALUE-ONLY model (abo_create) — the posterior of (f, ∇f) at M points under a GP
 * conditioned on function values alone, p = d + 1 outputs per point.  With J(z) = ∂k(X, z)/∂z (N × d), V = L⁻¹[k(X, z) J(z)]:
 *   mu[j] = (mean_c + k(X, z_j)ᵀalpha, J(z_j)ᵀalpha),   cov[j] = diag(sigma_f2, k″·I) − VᵀV,   k″ = −2·sigma_f2·φ'(0)/ell²
 * (the prior variance of a gradient output: sigma_f2/ell² SE, 5/3 of it Matérn-5/2, 7/5 Matérn-7/2).  mu [M][p], cov [M][p][p]
 * (point-major, symmetric, + 1e-18 on the diagonal as abo_predict_grad_cov adds it), score [M] = the GradientNormUCB value on the
 * gradient block exactly as abo_predict_grad_cov defines it; any of them may be NULL; Z in z_space, the outputs in out_space.
 * mu[j][0] and cov[j][0][0] are abo_predict's mean and variance to rounding.  M = 0 returns ABO_OK and writes nothing.
 * ABO_EINVAL, before any device work and with the call's name in abo_last_error: a null or unfitted handle; a gradient-enhanced
 * handle (abo_predict_grad_cov serves it); d not the model's; d > 32; the Matérn-3/2 family (the derivative blocks are built for the three
 * families a gradient-enhanced model takes); M < 0; a null Z with M > 0.
 * The contraction ALWAYS runs on the fp64 MFMA GEMM, whatever abo_set_contraction says (abo_timings.contraction_engine reports
 * ABO_CONTRACT_FP64): the int8-residue engine's per-row scaling for derivative query outputs on a value-only factor is a piece of work
 * of its own.  The result is the same bit for bit on every call and for every abo_params.chunk (a positive chunk caps the points per
 * chunk; otherwise V = p·N doubles per point stays within 256 MiB per chunk).  Works on appended views and after abo_remove, as
 * abo_predict does.  abo_timings: acq_kxz_ms the generator, acq_var_gemm_ms the GEMM, acq_finalize_ms the per-point epilogue.
 * Out of scope: multi-device handles (abo_mgpu_*) have no twin of this call; abo_acq_terms and the on-device refinement keep refusing a
 * GRADNORM_UCB term on a value-only handle; abo_optimize_acquisition is untouched.
 * Cost: p·M·N² flop for V (half of it skipped in the triangle) and p²·M·N/2 for the blocks; workspace 2·p·N doubles per point of a chunk. */
int32_t abo_predict_deriv(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, double beta,
                          double* mu, double* cov, double* score, int32_t out_space);

/* --- acquisition over a candidate batch -------------------------------------------------------
 * scores = acqf(surrogate, grid_points); sortperm(scores; rev=true)[1:k]
 * (src/acquisition_functions/acq_utils.jl:50-52) with the EI/UCB/PI epilogue fused behind the
 * posterior.  scores (length M) is optional; top_val/top_idx (length k) are optional when k == 0.
 * Ordering is Julia's stable reverse sort: descending score, ties → lowest index, NaN first.
 * top_idx are global indices idx_base + j (idx_base = this rank's shard offset).  k is free (n_local is a plain Int in
 * the reference, acq_utils.jl:33-38): k ≤ 1024 is one selection round, larger k takes ⌈k/1024⌉ rounds; when M < k the
 * tail is filled with (NaN, −1).  scores/top_* live in out_space. */
int32_t abo_acq(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, int32_t kind,
                double p0, double best_y, int64_t idx_base, double* scores, int32_t k,
                double* top_val, int64_t* top_idx, int32_t out_space);

/* abo_acq for a weighted-sum objective (EnsembleAcq.jl:53-55): the posterior is evaluated once, every member's epilogue runs on
 * it; with a GRADNORM_UCB term (gradient-enhanced handles) the per-point mean and covariance block of all outputs are evaluated
 * instead.  One term of weight 1 is abo_acq, bit for bit. */
int32_t abo_acq_terms(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, const abo_acq_term* terms,
                      int32_t nterms, int64_t idx_base, double* scores, int32_t k, double* top_val, int64_t* top_idx,
                      int32_t out_space);
/* the grid stage of optimize_acquisition (acq_utils.jl:44-52) on ONE handle, the grid never crossing PCIe: an n-point Latin
 * hypercube generated on the device (abo_lhs), scored, the k best returned — top_val / top_idx (k), top_x (k × d, optional: their
 * coordinates).  What abo_mgpu_acq_lhs is for a group.  Host outputs. */
int32_t abo_acq_lhs(abo_gp* gp, int64_t n, int32_t d, const double* lower, const double* upper, uint64_t seed, int32_t kind,
                    double p0, double best_y, int32_t k, double* top_val, int64_t* top_idx, double* top_x);

/* --- optimize_acquisition (src/acquisition_functions/acq_utils.jl:33-73) on the device -------------------------------
 * The reference: Latin-hypercube grid of n_grid points → scores → the n_local best as starts (:44-52) → for EVERY start one
 * box-constrained L-BFGS run, Fminbox(LBFGS(HagerZhang(linesearchmax = 20))) with Optim.Options(g_tol = 1e-5, f_abstol = 2.2e-9,
 * x_abstol = 1e-4), each objective value an M = 1 posterior call and each gradient a finite-difference stencil of them
 * (:55-71) → the best refined point (:66-72).
 * abo_refine is the second stage for S given starts: ONE launch, one workgroup per start running that start's whole projected
 * L-BFGS on the device — analytic ∇μ, ∇σ² from the kernel's derivative (∂k/∂x, L⁻¹, L⁻ᵀ), closed-form ∂EI/∂(μ,σ²) (UCB, PI
 * likewise), Armijo backtracking with at most linesearch_max trials, the reference's three stopping rules.  Maximises the
 * acquisition function inside the box [lower, upper].  x_out S × d, f_out S (the acquisition value at x_out: what abo_acq returns
 * for that point up to the rounding of a differently ordered sum), iters_out (optional) S × 2 = {iterations, evaluations}.  A start whose value is not finite
 * is returned unchanged.  All buffers HOST memory.
 * PARITY UNPINNED: the result is a local maximiser of the acquisition function in the box at the reference's tolerances — NOT Optim's
 * iterate.  The reference runs Fminbox (a log-barrier outer loop that keeps iterates strictly interior) around L-BFGS with HagerZhang
 * line searches and Optim's convergence bookkeeping; this is a projected L-BFGS with Armijo backtracking that may return a maximiser
 * ON the bound, and the reference holds no fixture of optimize_acquisition outputs.  What is tested: never below the start, inside
 * the box, at least SciPy L-BFGS-B's optimum on the CPU oracle's acquisition from the same start (tests/test_gpu_refine.py).
 * The option fields are clamped (max_iter ≤ 10000, linesearch_max ≤ 64, history ≤ 64).
 * Gradient-enhanced handles (ABI 5; the reference's tutorials drive optimize_acquisition with GradientGP, gradNormUCB.jl:39-51):
 * the starts advance in lockstep rounds; a round evaluates the all-output posterior of every pending point (the kernels of
 * abo_predict_grad_cov) and takes ∇μ = E[∇f(x)] − m_∇ and ∇σ² = 2·Cov(f(x), ∇f(x)) from it — the analytic gradient of EI / UCB /
 * PI at no extra cost; a GRADNORM_UCB term is differentiated by central differences over a 2d-point stencil evaluated in the same
 * batch (the reference differentiates every objective that way).
 * The *_terms forms take a weighted-sum objective (abo_acq_term: EnsembleAcquisition; ∇ = Σ w_t ∇acq_t on one posterior).
 * abo_optimize_acquisition is the whole function in ONE call: grid generated on the device (abo_lhs, `seed`), scored and
 * reduced to the min(n_local, n_grid) best (abo_acq), those refined, the best point returned: best_x (d), best_val; optional
 * starts_x (k × d) / starts_val (k): the selected grid points and their scores in selection order; refined_x / refined_val: what
 * each became.  The result is the refined point with the largest value (first one on ties, the reference keeps the first under
 * its strict `>`), or the best grid point if no refined value reaches its score. */
typedef struct abo_refine_opts {   /* NULL or zero fields = the reference's settings */
    int32_t max_iter;        /* L-BFGS iterations per start, 0 = 100 */
    int32_t linesearch_max;  /* trials per line search, 0 = 20 (acq_utils.jl:10) */
    int32_t history;         /* L-BFGS pairs kept, 0 = 10 (Optim's LBFGS default) */
    int32_t reserved;
    double g_tol, f_abstol, x_abstol;   /* 0 = 1e-5, 2.2e-9, 1e-4 (acq_utils.jl:62) */
} abo_refine_opts;
int32_t abo_refine(abo_gp* gp, int32_t kind, double p0, double best_y, const double* lower, const double* upper, int32_t d,
                   const double* starts, int32_t S, const abo_refine_opts* opts, double* x_out, double* f_out, int32_t* iters_out);
int32_t abo_optimize_acquisition(abo_gp* gp, int32_t kind, double p0, double best_y, const double* lower, const double* upper,
                                 int32_t d, int64_t n_grid, int32_t n_local, uint64_t seed, const abo_refine_opts* opts,
                                 double* best_x, double* best_val, double* starts_x, double* starts_val, double* refined_x,
                                 double* refined_val);
int32_t abo_refine_terms(abo_gp* gp, const abo_acq_term* terms, int32_t nterms, const double* lower, const double* upper, int32_t d,
                         const double* starts, int32_t S, const abo_refine_opts* opts, double* x_out, double* f_out,
                         int32_t* iters_out);
int32_t abo_optimize_acquisition_terms(abo_gp* gp, const abo_acq_term* terms, int32_t nterms, const double* lower,
                                       const double* upper, int32_t d, int64_t n_grid, int32_t n_local, uint64_t seed,
                                       const abo_refine_opts* opts, double* best_x, double* best_val, double* starts_x,
                                       double* starts_val, double* refined_x, double* refined_val);

/* --- resident candidate sets (BASELINE config 5: greedy q-EI over a fixed grid) --------------------
 * abo_cand_create copies M candidates to the device and evaluates their posterior with `gp`
 * (same arithmetic as abo_predict).  After `gp2 = abo_append(gp, x*, y*)`, abo_cand_downdate(gp2, c)
 * updates the stored posterior in O(N·M) instead of O(N²·M) — as one streaming pass over the K_ZX the set keeps
 * resident in HBM when M·N_max·8 bytes fit the budget (environment ABO_CAND_KZX_GIB, default 64; 0 = never), else
 * by re-evaluating the kernel:
 *   c(z) = k(z,x*) − k_zᵀK⁻¹k_*,   σ²(z) −= c(z)²/l_nn²,   μ(z) += c(z)·(y* − μ(x*))/l_nn²
 * (ABO_EINVAL if gp2 is not the one-point append of the model the set was last synced with).
 * abo_cand_acq runs the EI/UCB/PI/LOGEI epilogue + top-k of abo_acq on the stored posterior;
 * abo_cand_point returns one candidate's coordinates and posterior (host outputs, any may be NULL);
 * abo_cand_refresh re-evaluates from scratch (after a refit or a hyper-parameter change);
 * abo_cand_save / abo_cand_restore snapshot and roll back the stored posterior (greedy q-EI explores
 * fantasy appends, then the real observation is appended to the un-fantasised model). */
int32_t abo_cand_create(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, abo_cand** out);
int32_t abo_cand_destroy(abo_cand* c);
int32_t abo_cand_refresh(abo_gp* gp, abo_cand* c);
int32_t abo_cand_downdate(abo_gp* gp, abo_cand* c);
int32_t abo_cand_save(abo_gp* gp, abo_cand* c);
int32_t abo_cand_restore(abo_gp* gp, abo_cand* c);
int32_t abo_cand_acq(abo_gp* gp, abo_cand* c, int32_t kind, double p0, double best_y, int64_t idx_base,
                     double* scores, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space);
int32_t abo_cand_get(abo_gp* gp, abo_cand* c, double* mu, double* var, int32_t out_space);
int32_t abo_cand_point(abo_gp* gp, abo_cand* c, int64_t idx, double* x, double* mu, double* var);
/* takes candidate idx out of the running until the next refresh / restore: its stored posterior becomes (μ = +Inf,
 * σ² = 0), so EI = PI = 0 and UCB = −Inf there.  Greedy q-EI uses it (opt-in) to return q distinct points: with
 * observation noise the Kriging-believer fantasy does not collapse the variance at a picked point. */
int32_t abo_cand_exclude(abo_gp* gp, abo_cand* c, int64_t idx);

/* --- greedy (Kriging-believer) q-EI on a resident set, block form (ABI 6) -----------------------------------------
 * No reference counterpart (the reference's EI is single-point, src/acquisition_functions/ExpectedImprovement.jl:40-66, and its
 * update always refits, src/surrogates/StandardGP.jl:79-83): q × [EI over the grid → arg-max → condition the grid's posterior on
 * the fantasy observation (x_j, μ(x_j))] — each sub-step exactly `update` + EI semantics.  What a pick needs of
 * the resident K_ZX is one column of posterior covariances c_j(z) = Cov_{j−1}(z, x_j):
 *     Cov₀(z, x) = k(z, x) − k_zᵀK⁻¹k_x                                     under the model the set is synced with (the base),
 *     c_j(z) = Cov₀(z, x_j) − Σ_{i<j} c_i(z)·c_i(x_j)/s_i,   s_i = σ²_{i−1}(x_i) + σ²_n,   σ²_j(z) = σ²_{j−1}(z) − c_j(z)²/s_j
 * (μ is not touched: the fantasy value is the mean).  Cov₀ for a BLOCK of T points is ONE pass over K_ZX (a T-column product
 * on the fp64 matrix pipe under the 8·N·M-byte stream) where the plain loop (abo_append + abo_cand_downdate per pick) streams
 * K_ZX once per pick.  The block is the T best candidates of the current scores; a pick outside every block builds a new block
 * from the scores of that moment.  Nothing is appended to the model: on return model and set are as before (the batch is
 * rolled back), and the chain c_1 … c_{q−1} stays with the set — appending the picks for real, in order
 * (abo_append(gp, x_1, y_1) → abo_cand_downdate, …), finds each down-date column there instead of streaming K_ZX again
 * (c_j does not depend on the observed value).  Blocks and chain FOLLOW the model through real appends (any abo_cand_downdate puts
 * its column into the chain): the next batch, on the appended model, still finds the columns of the earlier blocks — a BO step's
 * picks are mostly the previous step's runners-up — corrected by the chain entries made since each block was built; a refresh,
 * another lineage of the model or 64 chain entries start the state afresh.
 *   abo_cand_qei: the whole batch on one handle.  x_out q × d, idx_out / ei_out q (idx = idx_base + local index);
 *     distinct != 0 excludes every picked candidate for the rest of the call; block = T (16 … 64, rounded up to a multiple of
 *     16; 0 = the process default, abo_set_qei_block / ABO_QEI_BLOCK, initially 32; < 0 = the plain loop).  The plain loop
 *     is also what runs for a gradient-enhanced model, for a set whose K_ZX is not resident, and for q > 64.  stats may be NULL.
 *   For a host that shards the set itself (one process per GPU: abstractbayesopt.jl_amd/incremental.py over torch.distributed)
 *   the same batch in steps; every shard makes the same calls with the same exchanged numbers, so a sharded set repeats the
 *   single set's arithmetic bit for bit:
 *     _begin(gp, c, q, block)                         snapshot σ², μ; empty chain and blocks
 *     _top(gp, c, xi, best_y, idx_base, k, rec)       EI over the shard and its k best as records of 4 + d + n doubles
 *                                                     {EI, global index (−1: none), μ, σ², x[0..d), c_1(x) … c_n(x)}, n = entries of the
 *                                                     chain (abo_cand_qei_has: real appends carried over + the batch's picks so far)
 *     _block(gp, c, pts, gidx, T)                     Cov₀ columns of T points (the merged best T of all shards) in one pass
 *     _pick(gp, c, gidx, var_x, cx, n, excl, info)    condition on the pick (its point must be in a block): var_x = σ²(x) and
 *                                                     cx[i] = c_{i+1}(x), i < n, both from the winner's record; excl ≥ 0: local index
 *                                                     to exclude; σ²(x) + noise ≤ 0 → ABO_ENOTPD, *info = N + n + 1 (the failed pivot
 *                                                     of the plain loop's bordered append)
 *     _end(gp, c)                                     roll σ², μ back; the chain stays for abo_cand_downdate */
typedef struct abo_qei_stats {
    int32_t picks, block, block_builds, block_hits;   /* block = T (0: the plain loop ran); hits: picks found in an existing block */
    double total_ms;                /* host wall clock of the call */
    double block_ms;                /* HIP events: all block builds of the batch (K⁻¹K_XT + the pass over K_ZX + kernel values) */
    double pass_ms;                 /* HIP events: the product over the resident K_ZX of the LAST block build */
    double pass_bytes, pass_flop;   /* algorithmic: 8·N·M bytes of K_ZX streamed once, 2·N·M·T flop */
} abo_qei_stats;
int32_t abo_set_qei_block(int32_t block);
int32_t abo_cand_qei(abo_gp* gp, abo_cand* c, int32_t q, double xi, double best_y, int32_t distinct, int64_t idx_base, int32_t block,
                     double* x_out, int64_t* idx_out, double* ei_out, abo_qei_stats* stats);
int32_t abo_cand_qei_begin(abo_gp* gp, abo_cand* c, int32_t q, int32_t block);
/* *ok = 1 when _begin(gp, c, q, block) would open a block-form batch on this shard (model fitted and in sync with the set, K_ZX
 * resident, q ≤ 64, block size > 0, …), 0 otherwise — the reason is then in abo_last_error.  Changes nothing.  Ranks that shard a set
 * themselves exchange this flag and take the block form only if EVERY rank can (a rank that cannot would leave the others'
 * all-gathers without a partner). */
int32_t abo_cand_qei_eligible(abo_gp* gp, abo_cand* c, int32_t q, int32_t block, int32_t* ok);
/* rec: k records of 4 + d + n doubles each, n = the chain's entries at the moment of the call (abo_cand_qei_has; it grows with
 * every pick and with the real appends carried over from earlier batches); cap_words = doubles the caller's buffer holds — ABO_EINVAL
 * (nothing written) when k·(4 + d + n) exceeds it.  A set's block slots are keyed by global index = idx_base + local index: every call
 * of one set passes the same idx_base (another value drops the blocks; the next pick builds a new one). */
int32_t abo_cand_qei_top(abo_gp* gp, abo_cand* c, double xi, double best_y, int64_t idx_base, int32_t k, double* rec, int64_t cap_words);
int32_t abo_cand_qei_block(abo_gp* gp, abo_cand* c, const double* pts, const int64_t* gidx, int32_t T);
int32_t abo_cand_qei_pick(abo_gp* gp, abo_cand* c, int64_t gidx, double var_x, const double* cx, int32_t n, int64_t excl,
                          int64_t* info);
int32_t abo_cand_qei_end(abo_gp* gp, abo_cand* c);
/* *has = 1 when candidate gidx is a point of one of the set's blocks; *nchain = entries of the set's chain (a record of _top carries
 * that many values behind x).  Either output may be NULL. */
int32_t abo_cand_qei_has(abo_gp* gp, abo_cand* c, int64_t gidx, int32_t* has, int32_t* nchain);
/* statistics of the set's current / last block-form batch (abo_cand_qei fills its own `stats` from the same numbers) */
int32_t abo_cand_qei_stats(abo_gp* gp, abo_cand* c, abo_qei_stats* out);

/* --- Monte-Carlo joint q-EI on a resident set (added within ABI 7) -------------------------------------------------------------
 * SURVEY.md §8 a13 (iii), the second definition of q-EI: the expectation over the JOINT posterior of the best improvement in the batch,
 * maximised greedily one point at a time (BoTorch's qExpectedImprovement with fixed base samples).  No reference counterpart; at q = 1
 * and S → ∞ it tends to the reference's EI (src/acquisition_functions/ExpectedImprovement.jl:40-66).
 * With μ(z), Cov(z, z') the posterior of the latent f under `gp` (which the set must be in sync with), the chain of the block form
 * above with NOISE-FREE pivots:
 *     c_i(z) = Cov(z, x_i) − Σ_{k<i} c_k(z)·c_k(x_i)/s_k,   s_i = v_{i−1}(x_i),   v_i(z) = v_{i−1}(z) − c_i(z)²/s_i,   v_0 = σ²(z)
 *     (a pick with s_i ≤ 1e-12 adds a zero column: the reference's EI threshold, ExpectedImprovement.jl:59)
 *     h_i(z) = c_i(z)/√s_i,   σ_j(z) = √v_{j−1}(z) if v_{j−1}(z) > 1e-12, else 0
 *     F^s_j(z) = μ(z) + Σ_{i<j} h_i(z)·ζ[s·q + i − 1] + σ_j(z)·ζ[s·q + j − 1]        (the sample s of f(z) when z is pick j)
 *     R^s_j = max(R^s_{j−1}, best_y − xi − F^s_j(x_j)),   R^s_0 = 0
 *     qEI_j(z) = (1/S)·Σ_s max(R^s_{j−1}, best_y − xi − F^s_j(z))              (s in order: repeated calls agree bit for bit)
 * Pick j is the arg-max of qEI_j over the set (ties: the lowest index, as abo_cand_qei); earlier picks and excluded candidates
 * (abo_cand_exclude: μ = +Inf) are never returned.  qei_out[j] = qEI_{j+1}(x_{j+1}), the joint q-EI of the first j + 1 picks: it never
 * decreases with j.  Everything is fp64.
 *   base: S × q standard normals, row-major (ζ[s·q + j]), in `base_space` — the caller's COMMON RANDOM NUMBERS: the same base gives
 *     the same batch, and two candidate batches compared under one base differ by their values, not by sampling noise.
 *   q 1 … 32, S 1 … 4096, block as abo_cand_qei (0 = the process default, else 16 … 64); x_out q × d, idx_out / qei_out q
 *   (idx = idx_base + local index); stats may be NULL.
 *   Only the block form exists: ABO_EINVAL (reason in abo_last_error) when K_ZX of the set is not resident, for a gradient-enhanced
 *   model, for a set out of sync with gp, or when the set holds fewer than q candidates that are not excluded.  Arguments (null
 *   pointers, values out of range, a non-finite host `base`) are checked before any device work.
 *   On return μ and σ² of the set are what they were, bit for bit, and the set's chain holds exactly the entries it held: the batch's
 *   noise-free entries are not down-date columns of a later noisy real append (abo_cand_downdate) and are never stored with the set.
 *   Blocks built during the call stay (they are Cov₀ under the set's model and serve a later abo_cand_qei as well). */
int32_t abo_cand_qei_mc(abo_gp* gp, abo_cand* c, int32_t q, double xi, double best_y, const double* base, int32_t S,
                        int32_t base_space, int64_t idx_base, int32_t block, double* x_out, int64_t* idx_out,
                        double* qei_out, abo_qei_stats* stats);

/* --- Thompson sampling: pathwise posterior sample paths (added within ABI 7) --------------------------------------------------
 * No reference counterpart (its acquisitions are EI, UCB, PI, GradientNormUCB and ensembles of them, src/acquisition_functions/): a
 * draw of a FUNCTION from the posterior, by pathwise conditioning (Matheron's rule; Wilson et al. 2020).  The reference minimises
 * (EI's best_y is minimum(ys), ExpectedImprovement.jl:81-83), so a Thompson pick is the arg-min of a path; a batch of q picks is q
 * arg-mins of independent paths and never touches σ².
 * Model: a fitted STANDARD GP handle — family, ℓ, σ_f², σ²_n = noise_var, mean c, points X (N × d), targets y and the factor of
 * K̃ = k(X,X) + σ²_n·I exactly as abo_fit / abo_append left it (a jittered factor is used as it is).  A gradient-enhanced handle:
 * ABO_EINVAL.  d ≤ 32 (the register-resident generator; beyond: ABO_EINVAL).
 * Base quantities, all fp64, supplied by the caller in `space` (ABO_HOST / ABO_DEVICE) — the result is a deterministic function of them:
 *     omega  R × d, point-major   frequencies of the UNIT-lengthscale kernel (the library divides by ℓ)
 *     phase  R                    in [0, 2π)
 *     w      S × R                N(0,1) feature weights
 *     eps    S × N                N(0,1) observation-noise draws
 *     φ_r(x) = sqrt(2σ_f²/R)·cos(ω_r·x/ℓ + phase_r)
 *     f_s(x) = c + Σ_r w[s, r]·φ_r(x)                                          (a prior draw in R random Fourier features)
 *     v_s    = K̃⁻¹(y − f_s(X) − sqrt(σ²_n)·eps[s, :])                         (N values per path)
 *     g_s(z) = f_s(z) + Σ_i k(z, x_i)·v_s[i]                                   (k = σ_f²·κ(‖z − x_i‖/ℓ), the library's own κ: the EXACT kernel row)
 * 1 ≤ S ≤ 256, 1 ≤ R ≤ 65536.  Arguments (null pointers, values out of range) are checked before the handle is looked at and before
 * any device work.
 *   abo_paths_create   conditions S paths: f_s(X) by the evaluation pass over the features alone, v_s = L⁻ᵀ(L⁻¹·) from the explicit
 *                      inverse factor the handle holds, O(N²·S).  The object RETAINS the model (abo_retain): it outlives abo_destroy of the
 *                      caller's own reference.  It describes the model it was created from: after gp2 = abo_append(gp, …) the paths of gp
 *                      are still paths of gp, the OLD model (make new ones from gp2); after abo_fit on the very handle `gp` — which replaces
 *                      that handle's model — abo_paths_eval returns ABO_EINVAL.
 *   abo_paths_eval     g_s over M candidates (Z point-major, d = the model's: else ABO_EDIM), one generated-operand product on the fp64
 *                      matrix pipe per chunk of candidates, O((N + R)·M·S); two calls with the same inputs return the same bits.
 *                      values (S × M, path-major: values[s·M + j]) is optional.  k ≥ 0 (free, as abo_acq's): per path the k candidates
 *                      with the SMALLEST g_s — abo_acq's ordering applied to score = −g_s (descending score, ties → lowest index, NaN
 *                      first, tail (NaN, −1) when M < k); top_val (S × k) holds g_s ITSELF (bit for bit values[s·M + top_idx − idx_base]; a NaN comes back as the quiet NaN 0x7ff8…),
 *                      top_idx (S × k) = idx_base + j.  values / top_* live in out_space.
 *   abo_paths_eval_cand  the same over a resident set's own coordinates; a candidate taken out by abo_cand_exclude (stored μ = +Inf) gets
 *                      g_s = +Inf.  The set need not be in sync with the model: only its coordinates and exclusions are read, nothing of it
 *                      is written.
 *   abo_paths_stats_get  HIP-event times of the last create / eval on the object, and the algorithmic flop 2·(N + R)·M·S of that eval. */
/* The paths object — S sample paths of ONE conditioned model, holding a reference to it — crosses the ABI as an untyped handle
 * (void*), which is what a host without the C type system binds anyway (Julia: Ptr{Cvoid}); only abo_paths_create makes one. */
typedef struct abo_paths_stats { double create_ms, eval_ms, eval_flop; int64_t S, R, N; } abo_paths_stats;
int32_t abo_paths_create(abo_gp* gp, int32_t S, int32_t R, const double* omega, const double* phase, const double* w,
                         const double* eps, int32_t space, void** out);
int32_t abo_paths_destroy(void* paths);
int32_t abo_paths_eval(void* paths, const double* Z, int64_t M, int32_t d, int32_t z_space, int64_t idx_base,
                       double* values, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space);
int32_t abo_paths_eval_cand(void* paths, abo_cand* c, int64_t idx_base, double* values, int32_t k, double* top_val,
                            int64_t* top_idx, int32_t out_space);
int32_t abo_paths_stats_get(void* paths, abo_paths_stats* out);

/* --- sample paths that FOLLOW the model through appends (added within ABI 7) ---------------------------------------------------
 * Pathwise conditioning has the structure of the bordered append.  With the new observation (x*, y*), u = K̃⁻¹k(X, x*),
 * s² = k(x*,x*) + σ²_n − k(X,x*)ᵀu (the append's pivot l_nn²) and ONE fresh N(0,1) draw ε*_s per path:
 *     a_s     = (y* − sqrt(σ²_n)·ε*_s − g_s(x*)) / s²          g_s(x*): the path BEFORE the append, at the new point
 *     v'_s    = [ v_s − a_s·u ;  a_s ]                          (N + 1 values per path)
 *     g'_s(z) = g_s(z) + a_s·c(z),   c(z) = k(z, x*) − k(z, X)·u
 * g'_s is the path abo_paths_create would build on the appended model from the same (omega, phase, w) and eps extended by the column
 * ε* — the block-inverse identity, nothing approximate.  u and s² are what abo_append left with the new handle, c(z) over a resident
 * set is the column abo_cand_downdate used: an append costs O((N + R)·S) for the object and O(M·S) for S resident values per
 * candidate, with no triangular mat-vec and no pass over the factor.
 * The advanced paths are exact posterior draws under the appended model, but they share their prior draw (omega, phase, w) with the
 * paths before the append — successive BO steps' paths are not independent of each other; a caller who wants fresh draws calls
 * abo_paths_create at its own cadence.
 *   abo_paths_append   advances the object IN PLACE from its model to gp2, which must be the ONE-point append of that model made by
 *                      abo_append: same factor storage, N(gp2) = N(paths) + 1.  A refit in disguise (the append fell back to a refit —
 *                      storage full or copy-on-write —, abo_fit), a handle more than one append ahead, another lineage, a
 *                      gradient-enhanced handle: ABO_EINVAL with the reason in abo_last_error, the object untouched.  k appends are k
 *                      calls, in append order.  eps_new: S doubles in `space` (a non-finite host value: ABO_EINVAL).  Every check comes
 *                      before any device work.  On success the object describes gp2: it retains gp2 and releases the old model (the
 *                      caller may abo_destroy its references to both), and abo_paths_eval / _eval_cand evaluate paths of the
 *                      appended model.  g_s(x*) is summed in a fixed order (no atomics): the same inputs give the same bits.
 *                      With a set attached (below) the set must be in sync with gp2 — abo_cand_downdate(gp2, c) has run; else
 *                      ABO_EINVAL, nothing changed — and the resident values follow: G[s][j] += a_s·c(z_j), in one launch that also
 *                      leaves each path's arg-min.  c(z) is read where the down-date left it (its pass's result, or the entry of the
 *                      set's q-EI chain it was served from) when that is certain, and recomputed with the down-date's own kernels
 *                      otherwise; a stale column is never used.
 *   abo_paths_attach   evaluates G[s][j] = g_s(z_j) over the set's candidates (the pass of abo_paths_eval_cand) and KEEPS it with the
 *                      object: S × M doubles of device memory (M rounded up to 1024); ABO_ENOMEM leaves the object unattached.  One
 *                      set per object (a second attach: ABO_EINVAL).  The object remembers the set but does not own it: the CALLER
 *                      keeps the set alive while it is attached; abo_paths_detach / abo_paths_destroy drop the values.
 *   abo_paths_top      selection over the resident values, the output contract of abo_paths_eval: top_val / top_idx are S × k in
 *                      out_space, per path the k candidates with the smallest g_s in abo_acq's order on −g_s (ties → lowest index,
 *                      NaN first, tail (NaN, −1) when M < k), top_idx = idx_base + j, top_val the bits of abo_paths_values at that
 *                      index.  A candidate taken out by abo_cand_exclude (stored μ = +Inf) counts as g = +Inf; exclusions are read
 *                      when the selection runs, not at attach time.  k = 1 returns what the fused reduction left after the last
 *                      attach / append without a further pass, unless the set's exclusions may have changed since (then the selection
 *                      alone is re-run); k > 1 is one abo_acq selection per path.
 *   abo_paths_values   the resident values, S × M path-major (values[s·M + j]), +Inf at excluded candidates.
 *   abo_paths_append_stats_get  the last abo_paths_append: HIP-event ms of (path values at x* + update of v) and of (column look-up or
 *                      recomputation + resident update + selection; 0 without a set), the algorithmic bytes 16·S·M + 8·M of the
 *                      latter, where the column came from (0: the down-date's pass, 1: the q-EI chain, 2: recomputed, −1: no set
 *                      or an empty one) and the number of appends the object has followed. */
typedef struct abo_paths_append_stats { double model_ms, resident_ms, resident_bytes; int64_t column_from_chain, appends; } abo_paths_append_stats;
int32_t abo_paths_append(void* paths, abo_gp* gp2, const double* eps_new, int32_t space);
int32_t abo_paths_attach(void* paths, abo_cand* c);
int32_t abo_paths_detach(void* paths);
int32_t abo_paths_top(void* paths, int64_t idx_base, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space);
int32_t abo_paths_values(void* paths, double* values, int32_t out_space);
int32_t abo_paths_append_stats_get(void* paths, abo_paths_append_stats* out);

/* --- grid generation and stand-alone epilogue (DEVICE buffers) --------------------------------------
 * abo_lhs: points j0 .. j0+count−1 of an n-point Latin-hypercube design in the box [lower, upper]
 * (QuasiMonteCarlo.sample(n, lower, upper, LatinHypercubeSample()), src/acquisition_functions/acq_utils.jl:44-47)
 * written point-major to Z_dev; counter-based (keyed Feistel permutation per coordinate), so each rank
 * generates its own shard and the candidate grid never crosses PCIe.  lower/upper: d host doubles.
 * abo_score: scores[j] = acq(mu[j], var[j]) — the EI / UCB / PI / MEAN / LOGEI epilogue on an existing posterior
 * (several acquisition functions on one posterior pass: EnsembleAcquisition, EnsembleAcq.jl:53-55). */
int32_t abo_lhs(int32_t device, int64_t n, int32_t d, const double* lower, const double* upper, uint64_t seed,
                int64_t j0, int64_t count, double* Z_dev);
int32_t abo_score(int32_t device, const double* mu, const double* var, int64_t M, int32_t kind, double p0,
                  double best_y, double* scores);

/* Max-value entropy search (ABO_ACQ_MES above), ABI 7.  ystar: S samples of the minimum value, 1 ≤ S ≤ 1024, in HOST or DEVICE memory
 * (ys_space; abo_refine_mes and abo_optimize_acquisition_mes: host) — what abo_paths_eval(…, k = 1) leaves in top_val for S sample
 * paths over a grid.  A null pointer, S out of range and a non-finite host sample return ABO_EINVAL before the handle is looked at;
 * StandardGP handles only (ABO_EINVAL for a gradient-enhanced one).  No abo_mgpu_* twins, and no MES member in an abo_acq_term sum.
 * abo_score_mes: scores[j] = MES(mu[j], var[j]) on an existing posterior (mu, var, scores: device buffers, as abo_score's).
 * abo_acq_mes: abo_acq with MES as the epilogue — one posterior pass, the epilogue on its μ, σ² (the same bits as abo_score_mes on
 * abo_predict's output), then abo_acq's selection: its order, idx_base, k > 1024 and the (NaN, −1) tail.  The pruned top-k selection
 * never applies (MES is not monotone in σ): abo_get_prune_stats reads all zeros afterwards.
 * abo_cand_acq_mes: the same on a resident set's stored posterior (abo_cand_acq).
 * abo_refine_mes / abo_optimize_acquisition_mes: abo_refine / abo_optimize_acquisition with MES as the objective (analytic gradient;
 * the samples are spread over the workgroup's lanes and summed in a fixed tree, so a refined value agrees with abo_acq_mes at the same
 * point to rounding, not bit for bit). */
int32_t abo_score_mes(int32_t device, const double* mu, const double* var, int64_t M, const double* ystar, int32_t S, int32_t ys_space,
                      double* scores);
int32_t abo_acq_mes(abo_gp* gp, const double* Z, int64_t M, int32_t d, int32_t z_space, const double* ystar, int32_t S, int32_t ys_space,
                    int64_t idx_base, double* scores, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space);
int32_t abo_cand_acq_mes(abo_gp* gp, abo_cand* c, const double* ystar, int32_t S, int32_t ys_space, int64_t idx_base, double* scores,
                         int32_t k, double* top_val, int64_t* top_idx, int32_t out_space);
int32_t abo_refine_mes(abo_gp* gp, const double* ystar, int32_t S, const double* lower, const double* upper, int32_t d,
                       const double* starts, int32_t n_starts, const abo_refine_opts* opts, double* x_out, double* f_out,
                       int32_t* iters_out);
int32_t abo_optimize_acquisition_mes(abo_gp* gp, const double* ystar, int32_t S, const double* lower, const double* upper, int32_t d,
                                     int64_t n_grid, int32_t n_local, uint64_t seed, const abo_refine_opts* opts, double* best_x,
                                     double* best_val, double* starts_x, double* starts_val, double* refined_x, double* refined_val);
/* monte_carlo_fill_distance (src/BO_utils.jl:140-159; the lower length-scale bound of optimize_hyperparameters,
 * src/BO_utils.jl:87-125): *out = max over the n_samples points S of the distance to the nearest of the N training points X
 * (both point-major, d coordinates; HOST or DEVICE memory each; out: one host double).  The caller draws the sample points — the
 * reference draws them with its own RNG in the box — so the result is the reference's for the same samples (ABI 7). */
int32_t abo_fill_distance(int32_t device, const double* X, int64_t N, int32_t d, int32_t x_space, const double* S, int64_t n_samples,
                          int32_t s_space, double* out);

/* --- scalars ----------------------------------------------------------------------------------
 * nlml (src/surrogates/StandardGP.jl:99-114) of the fitted state:
 * ½(N log 2π + logdet(K+noise I) + deltaᵀ alpha). */
int32_t abo_nlml(abo_gp* gp, double* out);

/* NLML and its analytic gradient with respect to (log ell, log sigma_f2) — what Optim's
 * `autodiff=:forward` computes with ForwardDiff duals in optimize_hyperparameters
 * (src/bayesian_opt.jl:253-285), which cannot cross a C-ABI:
 *   dNLML/dθ = ½ tr((K⁻¹ − ααᵀ) ∂K/∂θ),  K⁻¹ = L⁻ᵀL⁻¹ formed on the MFMA GEMM, ∂K/∂log ell generated on
 *   the fly (for a gradient-enhanced handle: generated as a matrix from the analytic derivative blocks of
 *   gradKernel, src/surrogates/GradientGP.jl:573-606, whose nlml is :684-698).  Needs a freshly fitted handle (not an
 *   appended view).  Any output may be NULL. */
int32_t abo_nlml_grad(abo_gp* gp, double* nlml, double* d_log_ell, double* d_log_sigma_f2);

/* added within ABI 7: the same call for a kernel with one length scale per coordinate (ARD),
 *   k(x,z) = sigma_f2·kappa(‖(x − z)./ℓ‖),  d_log_ell[c] = ½ tr((K⁻¹ − ααᵀ) ∂K/∂log ℓ_c)  for c < d,
 * evaluated at ℓ_c = the handle's ell for every c, all d traces in the one sweep over K⁻¹ − ααᵀ that abo_nlml_grad makes
 * (∂K_ij/∂log ℓ_c = sigma_f2·q(d2)·e_c², e = (x_i − x_j)/ell, d2 = Σ e_c², q = (∂kappa/∂log ell)/d2 in closed form).  Their sum is
 * abo_nlml_grad's d_log_ell up to the rounding of a differently ordered sum; nlml and d_log_sigma_f2 are abo_nlml_grad's bit for bit.
 * d_log_noise = ½·σ²·(tr K⁻¹ − αᵀα) with σ² the noise the factor was built with (0 when that is 0).
 *
 * The convention that makes this ARD: the library has ONE scalar ell, and an ARD model crosses this ABI as ell = 1 with every
 * coordinate pre-divided by its ℓ_c — training points, candidates and box bounds alike (abo_lhs in the scaled box is the scaled
 * design); returned points are multiplied back by ℓ_c.  On such a handle d_log_ell[c] is exactly ∂NLML/∂log ℓ_c.
 *
 * Needs a freshly fitted handle (not an appended view); d must be the model's (ABO_EDIM); a gradient-enhanced handle or d > 32 is
 * ABO_EINVAL; the arguments are checked before any device work.  abo_timings.nlml_kinv_ms / nlml_trace_ms are filled as by
 * abo_nlml_grad.  Any output may be NULL; d_log_ell holds d values.  Two calls on the same handle return the same bits. */
int32_t abo_nlml_grad_ard(abo_gp* gp, int32_t d, double* nlml, double* d_log_ell, double* d_log_sigma_f2, double* d_log_noise);

/* added within ABI 7: leave-one-out cross-validation (Rasmussen & Williams §5.4.2) from the resident W = L⁻¹ — no refit, no K⁻¹ product.
 * LOO predictive distribution of the N observed targets under the fitted model (noise included: it predicts y_i, not f(x_i)):
 *   B_ii = Σ_{k≥i} W_ki² (W = L⁻¹),  mu[i] = y_i − alpha_i/B_ii,  var[i] = 1/B_ii,
 *   lpd[i] = −½ log var[i] − (y_i − mu[i])²/(2 var[i]) − ½ log 2π,   *nlpl = −Σ_i lpd[i].
 * mu, var, lpd: N values in out_space (ABO_HOST / ABO_DEVICE), each may be NULL; nlpl: one host double, may be NULL.
 * O(N²): one read of the triangle of L⁻ᵀ.  Works on appended views as well as fresh fits (the sums stop at the view's own N: a parent
 * keeps returning its own values after a child was appended); the noise is the one the factor was built with, y_i the target as
 * handed over.  A gradient-enhanced handle is ABO_EINVAL (leaving out one output row of a point is not LOO), as are a null or an
 * unfitted handle; the arguments are checked before any device work.  Two calls on the same handle return the same bits. */
int32_t abo_loo(abo_gp* gp, double* mu, double* var, double* lpd, double* nlpl, int32_t out_space);

/* nlpl and its gradient with respect to (log ell, log sigma_f2, log noise); any output may be NULL.
 *   ∂(−nlpl)/∂θ = Σ_i [α_i r_i − ½(1 + α_i²/B_ii) s_i]/B_ii,  r = B (∂K/∂θ) α,  s_i = [B (∂K/∂θ) B]_ii,  B = K⁻¹ (all of it: the lower
 * 128-tiles of WᵀW on the fp64 MFMA GEMM, mirrored), ∂K/∂log ell generated as a matrix and multiplied once (one full N³ product);
 * the sigma_f2 and noise partials take no product (∂K = K − noise·I and noise·I).  d_log_noise is exactly 0 when the factor was built
 * without noise.  nlpl is abo_loo's bit for bit.  Needs a freshly fitted handle (not an appended view), as abo_nlml_grad does. */
int32_t abo_loo_grad(abo_gp* gp, double* nlpl, double* d_log_ell, double* d_log_sigma_f2, double* d_log_noise);

/* added within ABI 7: joint posterior covariance between two point sets — cov(gpx(Za), gpx(Zb)) and mean_and_cov of AbstractGPs (the
 * reference itself calls cov(model.gpx(…)) in posterior_grad_cov, GradientGP.jl:966-971):
 *   cov[i][j] = sigma_f2·kappa(‖za_i − zb_j‖/ell) − Σ_k V_a[k][i]·V_b[k][j],   V = L⁻¹K_XZ,
 * row-major Ma × Mb, the LATENT covariance (no observation noise: abo_predict's convention); mu_a (Ma) and mu_b (Mb) are abo_predict's
 * means, bit for bit.  mu_a, mu_b and cov may each be NULL.  Za / Zb in z_space, the outputs in out_space (ABO_HOST / ABO_DEVICE).
 * Zb == NULL is the symmetric form cov(Za, Za): Mb must be 0 or Ma and mu_b NULL (ABO_EINVAL otherwise); the result is symmetric bit for
 * bit (the lower 128-tiles are computed — half the flop — and mirrored) and its diagonal carries abo_predict's + 1e-18.  The rectangular
 * form with Zb = Za agrees with it to rounding and carries no jitter.
 * 1 ≤ Ma, Mb ≤ 8192; d must be the model's (ABO_EDIM); a null, an unfitted or a gradient-enhanced handle is ABO_EINVAL (its per-point
 * block is abo_predict_grad_cov's); every argument is checked before any device work.
 * The call ALWAYS runs on the fp64 MFMA kernels, whatever abo_set_contraction says: the int8-residue engine contracts the squares of
 * one operand (the column norms of V), and its error analysis — row scales against the L1 norm of each row of L⁻¹, a non-negative
 * sum — does not cover the signed cross products V_aᵀV_b.  The same bits under either engine setting, and on every call.
 * Works on appended views and on a parent after a child was appended: the columns of V beyond the view's own N are zeroed before the
 * product (rows ≥ N of shared factor storage may hold a discarded branch).  Cost: (Ma + Mb)·N² flop for the V's (half of that skipped
 * in the triangle) and 2·Ma·Mb·N for the product; workspace (Ma + Mb)·N + Ma·Mb doubles (padded to 128), cached on the handle. */
int32_t abo_predict_cov(abo_gp* gp, const double* Za, int64_t Ma, const double* Zb, int64_t Mb, int32_t d, int32_t z_space, double* mu_a,
                        double* mu_b, double* cov, int32_t out_space);

/* added within ABI 7: knowledge gradient over a discrete decision set (Frazier, Powell and Dayanik 2009; with ABO_KG_SELF the KGCP of Scott
 * et al. 2011) — the expected decrease of the minimum of the posterior mean over the decision set Zb from ONE observation at a candidate
 * za_i (minimisation, as every acquisition here):
 *   KG_i = min_j mu_j − E[min_j (mu_j + s_ij·Z)] = E[max_j (a_j + b_ij·Z)] − max_j a_j >= 0,   Z ~ N(0, 1),
 *   a_j = −mu(zb_j),   b_ij = s_ij = cov(f(za_i), f(zb_j)) / sqrt(v_i + noise),   v_i = var f(za_i)  (latent, + 1e-18 as abo_predict's).
 * Exact: per candidate the Mb lines sorted by (b, a), of equal slopes the largest intercept kept, one scan for the upper envelope
 * e_0 … e_m with breakpoints c_1 … c_m, KG = Σ_t (b_{e_t} − b_{e_{t−1}})·h(−|c_t|), h(z) = phi(z) + z·Phi(z) — every term >= 0, summed in
 * envelope order.  It needs no best_y and no xi or beta.  mu and the covariance are abo_predict_cov's (the means abo_predict's bit for
 * bit); the Ma × Mb block stays on the device: one number per candidate comes back.
 * Zb == NULL is the symmetric form: the decision set is Za itself (Mb must be 0 or Ma), the covariance the half-product plus mirror,
 * v_i its diagonal; row i's own point is in the set.  With Zb given, flags = ABO_KG_SELF adds the candidate's own line
 * (a = −mu(za_i), b = v_i / sqrt(v_i + noise)) to row i — what one wants when Zb is the training set; the flag is ABO_EINVAL in the symmetric
 * form, as is any other bit.  noise < 0: the noise the factor was built with (abo_loo's); noise >= 0 as given; NaN or Inf: ABO_EINVAL.
 * Degenerate rows: v_i + noise <= 1e-12 gives exactly 0.0 (the sigma² <= 1e-12 branch of the EI / PI epilogues); one line, or all slopes
 * equal, gives exactly 0.0; a non-finite mean or covariance in the row gives NaN.
 * scores (Ma values, may be NULL) and the k selected pairs (top_val, top_idx + idx_base; Julia's stable reverse order: descending, ties to
 * the lowest index, NaN first; (NaN, −1) behind Ma < k) in out_space; Za / Zb in z_space.
 * 1 <= Ma, Mb <= 8192; d must be the model's (ABO_EDIM); a null, an unfitted or a gradient-enhanced handle is ABO_EINVAL; every argument is
 * checked before any device work.  Always on the fp64 MFMA kernels, for abo_predict_cov's reason: the same bits on every call and under
 * either abo_set_contraction setting.  Works on appended views and on a parent after a child was appended, as abo_predict_cov does.
 * Cost: abo_predict_cov's, plus per candidate a sort of Mb pairs in LDS and a sequential envelope scan of Mb steps by one lane. */
enum { ABO_KG_SELF = 1 };
int32_t abo_acq_kg(abo_gp* gp, const double* Za, int64_t Ma, const double* Zb, int64_t Mb, int32_t d, int32_t z_space, double noise,
                   int32_t flags, int64_t idx_base, double* scores, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space);

/* --- introspection (tests) ----------------------------------------------------------------------
 * L (N×N row-major, strictly-upper part zero), alpha (N), Linv = L⁻¹ (N×N row-major); any may be
 * NULL.  Host buffers. */
int32_t abo_get_factor(abo_gp* gp, double* L, double* alpha, double* Linv);
int32_t abo_get_n(abo_gp* gp, int64_t* N, int32_t* d);
/* the training data the model is conditioned on, back to host buffers: X (points × d, point-major) and y (factor rows:
 * one per point, or p per point ordered by outputs for a gradient-enhanced model).  The reference keeps no
 * serialisation code; its BOStruct is rebuilt from (xs, ys, hyper-parameters) (src/bayesian_opt.jl:81,:163-165) —
 * this is the device-side half of that: checkpoint = hyper-parameters + these arrays, resume = abo_fit. */
int32_t abo_get_data(abo_gp* gp, double* X, double* y);
int32_t abo_get_timings(abo_gp* gp, abo_timings* out);
int32_t abo_get_prune_stats(abo_gp* gp, abo_prune_stats* out);
/* added within ABI 7: the bound levels of the same call.  out[6] = {rows of level 1 (0: the call had no first level — then all six are
 * 0 and abo_prune_stats describes its one bound pass), S₁ = candidates whose level-1 bound reached the threshold, rows of level 2
 * (0: skipped, S₁ ≤ 4·K₀ went straight to the full contraction), S₂ = of those S₁ the ones whose level-2 bound reached it too (0 when
 * skipped), time of level 1, time of level 2} — the two times in whole MICROSECONDS (HIP events on the handle's stream; level 2's
 * includes gathering its points and compacting again). */
int32_t abo_get_prune_levels(abo_gp* gp, int64_t* out);

/* --- multi-device handles (BASELINE configs 4 and 5: candidates sharded over the GPUs of one node) -----------------
 * One host process drives all devices: the Julia host has no process launcher, so the sharding of
 * `scores = acqf(surrogate, grid)` + `sortperm(scores; rev=true)[1:n_local]` (src/acquisition_functions/acq_utils.jl:50-52)
 * happens inside the library.  An abo_mgpu owns one abo_gp per listed device (a device may be listed more than once: each
 * entry is one shard).  Every device fits the same model redundantly (deterministic kernels → bit-identical factors; the
 * refit is ≈1 % of a config-3 step), candidates are cut into contiguous shards (sizes differ by at most one, earlier
 * shards take the larger ones), one host thread per shard drives its device, and the only exchange is the selection: each
 * device's k × (score, global index) go through ONE ncclAllGather (RCCL over xGMI; RCCL has no MAXLOC) and are merged in
 * the reference's order — descending score, ties → lowest index, NaN first — so the result equals the single-device
 * abo_acq on the whole batch bit for bit.  RCCL is loaded at run time (librccl.so.1, whichever copy the process already
 * has); when it is missing, fails to initialise, or the list names one device twice (RCCL refuses that), the pairs are
 * copied to the host per device instead — same merge, same result (abo_mgpu_info tells which).  Environment
 * ABO_MGPU_EXCHANGE = host | rccl overrides the choice (rccl on a one-entry list exercises the RCCL calls at world size 1).
 * All buffers of these entry points are HOST memory.  A handle is not re-entrant. */
typedef struct abo_mgpu abo_mgpu;     /* opaque: one model replicated on ndev devices */
typedef struct abo_mcand abo_mcand;   /* opaque: a candidate set sharded over those devices, resident with its posterior */
enum { ABO_XCHG_HOST = 0, ABO_XCHG_RCCL = 1 };

/* HipStandardGP(kernel, noise_var; mean, devices = [...]) — params->device is ignored, dev[0..ndev) are the HIP ordinals,
 * 1 ≤ ndev ≤ 16 */
int32_t abo_mgpu_create(const abo_params* params, int32_t ndev, const int32_t* dev, abo_mgpu** out);
/* the same for the gradient-enhanced model (abo_create_grad on every device: GradientGP(kernel, p, noise_var; mean), GradientGP.jl:
 * 617-639).  abo_mgpu_fit then takes y of length p·N ordered by outputs, abo_mgpu_predict / _acq / _acq_lhs / _cand_* address the
 * function output, abo_mgpu_append_grad appends one observation {f, ∂f/∂x_1 …} on every device (abo_append_grad), and
 * abo_mgpu_cand_qei conditions each pick on the posterior mean of all p outputs at the picked point (the Kriging-believer fantasy of a
 * model that observes gradients). */
int32_t abo_mgpu_create_grad(const abo_params* params, int32_t p, const double* mean_c, int32_t ndev, const int32_t* dev, abo_mgpu** out);
/* Base.copy (StandardGP.jl:26): a new group sharing every per-device state (abo_retain) */
int32_t abo_mgpu_clone(abo_mgpu* mg, abo_mgpu** out);
int32_t abo_mgpu_destroy(abo_mgpu* mg);
/* ndev, the device list (16 entries, may be NULL) and the exchange transport in use (ABO_XCHG_*) */
int32_t abo_mgpu_info(abo_mgpu* mg, int32_t* ndev, int32_t* dev, int32_t* exchange);
/* the per-device handle of shard i (borrowed: valid until the next abo_mgpu_fit / abo_mgpu_append / abo_mgpu_destroy):
 * abo_get_factor, abo_get_timings, abo_nlml, abo_nlml_grad … apply to it */
int32_t abo_mgpu_get(abo_mgpu* mg, int32_t i, abo_gp** out);
/* update(model, xs, ys): the same full refit on every device, concurrently (abo_fit) */
int32_t abo_mgpu_fit(abo_mgpu* mg, const double* X, int64_t N, int32_t d, const double* y, int64_t* info);
/* posterior_mean / posterior_var over M candidates, shard i computed on device i (abo_predict) */
int32_t abo_mgpu_predict(abo_mgpu* mg, const double* Z, int64_t M, int32_t d, double* mu, double* var);
/* abo_acq over M candidates sharded across the devices; scores (M, optional) land in the caller's array shard by shard,
 * top_val / top_idx (k) are the merged global selection with 0-based indices into Z */
int32_t abo_mgpu_acq(abo_mgpu* mg, const double* Z, int64_t M, int32_t d, int32_t kind, double p0, double best_y,
                     double* scores, int32_t k, double* top_val, int64_t* top_idx);
/* the grid stage of optimize_acquisition (acq_utils.jl:44-52) without the candidates ever crossing PCIe: device i generates
 * its shard of the n-point Latin-hypercube design (abo_lhs), scores it and selects; top_x (k × d, optional) receives the
 * coordinates of the selected points */
int32_t abo_mgpu_acq_lhs(abo_mgpu* mg, int64_t n, int32_t d, const double* lower, const double* upper, uint64_t seed,
                         int32_t kind, double p0, double best_y, int32_t k, double* top_val, int64_t* top_idx, double* top_x);
/* BASELINE config 5 across devices.  abo_mgpu_append: every device applies the same bordered append (abo_append) and the
 * group moves on to the N+1-point model (clone first to keep the old one); a candidate set, if given, is down-dated in the
 * same call (abo_cand_downdate).  abo_mgpu_cand_create / _lhs: shard a candidate grid over the devices and evaluate its
 * posterior; _refresh after a refit.  abo_mgpu_cand_acq: epilogue + merged top-k on the stored posterior.
 * abo_mgpu_cand_qei: greedy (Kriging-believer) q-EI — q × [EI + arg-max per device, ONE all-gather of the devices' pick
 * records] with the grid conditioned on each pick (y = μ(x): variances only) before the next; on return model and set are as
 * before.  ABI 6: the block form of abo_cand_qei run across the shards whenever every shard qualifies — per batch the shards'
 * top-T are gathered, every shard forms the covariance columns of the SAME T block points in one pass over its part of K_ZX
 * and conditions on a pick by a rank-1 correction from the chain of earlier picks' columns (records {EI, index, μ, σ², x,
 * chain values}); no fantasy append, no pass per pick; blocks and chain stay with the set from call to call
 * (abo_mgpu_cand_qei_stats).  Otherwise (a shard without room for the block buffers, a gradient-enhanced model, q > 64): the
 * plain loop — the same fantasy append (y = μ(x)) and O(N·M) down-date on every device between picks (q − 1 of them: the last
 * pick conditions nothing), rolled back at the end.  Both give the same picks as one handle over the whole set.  x_out q × d,
 * idx_out / ei_out q.  distinct != 0 excludes every picked candidate for the rest of the call. */
int32_t abo_mgpu_append(abo_mgpu* mg, const double* x, int32_t d, double y, int64_t* info, abo_mcand* cands);
int32_t abo_mgpu_append_grad(abo_mgpu* mg, const double* x, int32_t d, const double* y, int64_t* info, abo_mcand* cands);
/* abo_update for a group: the same rule, the prefix compared on the group's first device (the data is replicated); then a clone of
 * `prev` moves through the k appends (abo_mgpu_append / _append_grad), or a new group on prev's device list is created and fitted
 * (abo_mgpu_create(_grad) + abo_mgpu_fit; params->device is ignored).  `prev` is never mutated.  Host buffers only. */
int32_t abo_mgpu_update(abo_mgpu* prev, const abo_params* params, const double* mean_c, const double* X, int64_t N, int32_t d,
                        const double* y, int64_t* info, int32_t* path, abo_mgpu** out);
/* abo_optimize_acquisition across the group's devices: the grid stage as abo_mgpu_acq_lhs (shards generated, scored and reduced
 * on their devices, ONE all-gather of the selections), then the selected starts are dealt out contiguously and every device
 * refines its share with abo_refine's launch; a start's refinement does not depend on which device runs it, so the result equals
 * the single-device call with the same seed bit for bit. */
int32_t abo_mgpu_optimize_acquisition(abo_mgpu* mg, int32_t kind, double p0, double best_y, const double* lower, const double* upper,
                                      int32_t d, int64_t n_grid, int32_t n_local, uint64_t seed, const abo_refine_opts* opts,
                                      double* best_x, double* best_val, double* starts_x, double* starts_val, double* refined_x,
                                      double* refined_val);
int32_t abo_mgpu_optimize_acquisition_terms(abo_mgpu* mg, const abo_acq_term* terms, int32_t nterms, const double* lower,
                                            const double* upper, int32_t d, int64_t n_grid, int32_t n_local, uint64_t seed,
                                            const abo_refine_opts* opts, double* best_x, double* best_val, double* starts_x,
                                            double* starts_val, double* refined_x, double* refined_val);
int32_t abo_mgpu_cand_create(abo_mgpu* mg, const double* Z, int64_t M, int32_t d, abo_mcand** out);
int32_t abo_mgpu_cand_create_lhs(abo_mgpu* mg, int64_t n, int32_t d, const double* lower, const double* upper, uint64_t seed,
                                 abo_mcand** out);
int32_t abo_mgpu_cand_refresh(abo_mgpu* mg, abo_mcand* mc);
int32_t abo_mgpu_cand_destroy(abo_mcand* mc);
int32_t abo_mgpu_cand_acq(abo_mgpu* mg, abo_mcand* mc, int32_t kind, double p0, double best_y, int32_t k, double* top_val,
                          int64_t* top_idx);
/* the stored posterior of the whole sharded set in the candidates' global order (abo_cand_get shard by shard; mu / var: M host
 * doubles each, either may be NULL) */
int32_t abo_mgpu_cand_get(abo_mgpu* mg, abo_mcand* mc, double* mu, double* var);
int32_t abo_mgpu_cand_qei(abo_mgpu* mg, abo_mcand* mc, int32_t q, double xi, double best_y, int32_t distinct, double* x_out,
                          int64_t* idx_out, double* ei_out);
/* statistics of the last abo_mgpu_cand_qei on this set (shard 0's; block = 0 when the plain loop ran).  ABI 6: abo_mgpu_cand_qei
 * runs the block form (abo_cand_qei's; block size = the process default) whenever every shard qualifies, the plain loop else. */
int32_t abo_mgpu_cand_qei_stats(abo_mgpu* mg, abo_mcand* mc, abo_qei_stats* out);

/* --- memory -----------------------------------------------------------------------------------
 * Device buffers of destroyed handles are cached per device (update() makes a new model every BO
 * step and drops the old one, src/surrogates/StandardGP.jl:82 / src/bayesian_opt.jl:116-125) and
 * reused by the next handle; this returns the cached blocks of one device to the driver.  The cache
 * is bounded by the environment variable ABO_POOL_LIMIT_MB (default 32768). */
int32_t abo_pool_trim(int32_t device);

/* --- errors / version ---------------------------------------------------------------------------*/
/* copies the calling thread's last error text (NUL-terminated, truncated to cap) */
int32_t abo_last_error(char* buf, size_t cap);
int32_t abo_abi_version(void);

/* --- building blocks exposed for tests and profiling (all buffers DEVICE memory) ------------------
 * NOT part of the shipped ABI: compiled only into the test build of the library (-DABO_TEST_HOOKS:
 * abstractbayesopt.jl_amd/lib/libabo_hip_test.so, what the GPU suite loads); libabo_hip.so exports none of them. */
#ifdef ABO_TEST_HOOKS
/* The host-side decisions of the pruned top-k selection (no GPU needed) for a model of `rows` factor rows and p_out outputs per
 * point: out[4] = {eligible, 256-row blocks of the bound pass, K₀, largest survivor count that still takes the survivor pass}. */
int32_t abo_test_prune_plan(int64_t rows, int64_t M, int32_t k, int32_t want_scores, int32_t kind, double p0, int32_t p_out,
                            int32_t int8_fused, int32_t d, int64_t* out);
/* Process-wide overrides for tests and measurements: rblocks > 0 = that many row blocks in the bound pass instead of the rule's;
 * mode 1 = a threshold of −Inf (every candidate survives: the selection's worst case on any data), mode 2 = the path is off, as under
 * ABO_ACQ_PRUNE=0.  (0, 0) restores the defaults. */
int32_t abo_test_prune_force(int32_t rblocks, int32_t mode);
/* The same for the first bound level: pre_rblocks −1 = no first level (the call has one bound pass, over the rule's or the forced
 * row blocks), 0 = the rule (N/32 where that is fewer blocks than the bound pass's and abo_test_prune_force forces none), > 0 = that
 * many row blocks — an abo_acq whose bound pass has no more row blocks than that then fails with ABO_EINVAL.  level2_min −1 = the rule
 * (level 2 runs on more than 4·K₀ survivors of level 1), ≥ 0 = on more than level2_min of them (0: always).  (0, −1) restores the defaults. */
int32_t abo_test_prune_levels(int32_t pre_rblocks, int64_t level2_min);
/* The tail of the mean in the FIRST bound level (csrc/kgen_tail32.hip), process-wide: 1 = in fp32, 0 = in fp64 as every other bound
 * pass has it (ABO_PRUNE_TAIL32=0), −1 restores the environment's choice.  Nothing in a call without a first level. */
int32_t abo_test_prune_tail32(int32_t mode);
/* Survivors that the threshold pass has already scored (no second level ran, k ≤ S ≤ K₀), process-wide: 1 = their scores are taken from
 * that pass, 0 = the survivor pass evaluates them again (ABO_PRUNE_REUSE=0), −1 restores the environment's choice. */
int32_t abo_test_prune_reuse(int32_t mode);
/* *out = 1 when the last abo_acq on this handle took its survivors' scores from its threshold pass, else 0. */
int32_t abo_test_prune_reused(abo_gp* g, int32_t* out);
/* The HEAD of that first level (csrc/kgen_head32.hip), process-wide: 1 = head of the mean and guarded sum of squares by the fused
 * fp32-MFMA kernel, 0 = on the int8 engine (ABO_PRUNE_HEAD32=0), −1 restores the environment's choice.  The fused head runs only where
 * the fp32 tail does, and never under an explicit moduli request (ABO_PRUNE_BOUND_MODULI, abo_test_prune_bound_moduli != 0). */
int32_t abo_test_prune_head32(int32_t mode);
/* Preparation and kernel of the fused head alone, on a fitted ordinary model, over its first 256·rblocks rows (≤ N) and the M HOST
 * candidates Z [M][d]: head and ssq (M + 1 doubles each), delta and l1 (256·rblocks + 1 each).  The last entry of each is a sentinel (−7)
 * the kernels must leave alone. */
int32_t abo_test_bound_head32(abo_gp* g, const double* Z, int64_t M, int32_t rblocks, double* head, double* ssq, double* delta, double* l1);
/* abo_test_prune_plan with out[5]: the same four values, then the 256-row blocks of the first level (0: none).  ABO_EINVAL for a forced
 * first level that is not below the bound pass's row blocks.  No GPU needed. */
int32_t abo_test_prune_plan_levels(int64_t rows, int64_t M, int32_t k, int32_t want_scores, int32_t kind, double p0, int32_t p_out,
                                   int32_t int8_fused, int32_t d, int64_t* out);
/* Moduli of the bound pass's residue plan, process-wide: 8, 9, 10 = a short plan with the guard of csrc/ozaki.hip ("the guarded
 * bound"), 14 = the handle's plan, exact; 0 restores ABO_PRUNE_BOUND_MODULI / the default (8). */
int32_t abo_test_prune_bound_moduli(int32_t n);
/* sexp_b[0..n_rows), delta[0..n_rows) (host) = the row scales s_i and the guards delta[i] of the short plan the last abo_acq on this
 * handle ran its LAST bound pass on (n_rows ≤ 256 × its row blocks; with two levels: the second when it ran); an error when that pass
 * ran on the handle's own plan */
int32_t abo_test_prune_bound_plan(abo_gp* gp, int32_t* sexp_b, double* delta, int64_t n_rows);
/* out[0..M) (host) = the upper bounds the last abo_acq on this handle stored in its bound pass: the score at (μ̃ − ε, σ²_R) plus the
 * margins of prune_keep (csrc/misc.hip), so that each is ≥ the full pass's computed score of the candidate.  With two levels: the
 * first level's bound, lowered to the second level's where that pass looked at the candidate */
int32_t abo_test_prune_bounds(abo_gp* gp, double* out, int64_t M);
/* mu[0..M), eps[0..M) (host) = the mean μ̃ the last abo_acq on this handle computed in its bound pass (first row blocks' columns by the
 * full generator, the others by the shortened sequences of csrc/kgen_tail.hip) and the distance ε it proved to the full pass's mean:
 * the bounds above are scores at μ̃ − ε */
int32_t abo_test_prune_mean(abo_gp* gp, double* mu, double* eps, int64_t M);
/* head[0..M), ssq[0..M) (host) = what the fused head of the first bound level (csrc/kgen_head32.hip) wrote for every candidate in the
 * last abo_acq on this handle: the head of the mean and the guarded sum of squares; an error when that call ran no fused head */
int32_t abo_test_prune_head(abo_gp* gp, double* head, double* ssq, int64_t M);
/* out[i] = kappa_tail(family, d2[i]): the shortened kernel evaluation of that pass (csrc/abo_kappa.h), without sigma_f2 */
int32_t abo_test_kappa_tail(int32_t device, int32_t family, const double* d2, double* out, int64_t n);
/* out[i] = kappa_tail32(family, d2[i] rounded to fp32): the fp32 evaluation of the first level's tail (csrc/abo_kappa.h), without
 * sigma_f2; NaN where the two halves of the packed pair disagree */
int32_t abo_test_kappa_tail32(int32_t device, int32_t family, const double* d2, double* out, int64_t n);
/* The int8-residue engine's host constants for n moduli (no GPU needed): p[16] moduli, tables[4][16] = {1/p, 2^26 mod p
 * (symmetric), head and tail of (P/p)·((P/p)⁻¹ mod p)}, scal[3] = {head of P, tail of P, 1/P}, *eP with 2^eP ≤ P/4. */
int32_t abo_test_oz_plan(int32_t n, int32_t* p, double* tables, double* scal, int32_t* eP);
/* partial[tb][j] = Σ_{i in 128-row block tb, i < nvalid} (Σ_{k ≤ i} W[i][k]·Kxz[j][k])² through the int8-residue engine's own
 * quantisers, GEMM and reconstruction, for ANY lower-triangular W [Np][ldw] and any Kxz [Mc][ldk] with |Kxz| ≤ kmax (device
 * buffers; Np, Mc multiples of 128; partial [Np/128][ldp]). */
int32_t abo_test_oz_contract(int32_t device, const double* W, int64_t ldw, int32_t Np, int32_t nvalid, const double* Kxz, int64_t ldk,
                             int32_t Mc, double kmax, int32_t nmod, double* partial, int64_t ldp);
/* The same for the first 256·rblocks rows of W on the SHORT plan of the pruned selection's bound pass (nmod_b moduli, the bit split
 * and the guard of csrc/ozaki.hip, "the guarded bound"): partial[tb][j] for tb < 2·rblocks = Σ max(|Ṽ_ij| − delta[i], 0)², and
 * delta[0 .. 256·rblocks) (device) the guards; every entry ≤ what abo_test_oz_contract writes there with 14 moduli, NaN for a 128-row
 * block that holds a non-finite row of W.  kmax bounds Kxz up to the factor 1 + 2^-40. */
int32_t abo_test_oz_contract_bound(int32_t device, const double* W, int64_t ldw, int32_t Np, int32_t nvalid, const double* Kxz, int64_t ldk,
                                   int32_t Mc, double kmax, int32_t nmod_b, int32_t rblocks, double* partial, int64_t ldp, double* delta);
/* f[j], grad[j][0..d) = value and analytic gradient of the acquisition function at Z[j] (host buffers, M × d): the evaluation
 * the refinement stage is built on, one workgroup per point */
int32_t abo_test_acq_grad(abo_gp* gp, int32_t kind, double p0, double best_y, const double* Z, int64_t M, int32_t d, double* f,
                          double* grad);
int32_t abo_test_acq_grad_terms(abo_gp* gp, const abo_acq_term* terms, int32_t nterms, const double* Z, int64_t M, int32_t d,
                                double* f, double* grad);
/* f[j], dmu[j], dvar[j] = value and partial derivatives ∂/∂μ, ∂/∂σ² of the epilogue `kind` (as abo_score's) at mu[j], var[j] (device
 * buffers): the closed-form partials that gradient is assembled from */
int32_t abo_test_acq_partials(int32_t device, const double* mu, const double* var, int64_t M, int32_t kind, double p0, double best_y,
                              double* f, double* dmu, double* dvar);
/* the same two hooks for max-value entropy search (ystar: S samples; device memory for the partials, host memory for the gradient) */
int32_t abo_test_mes_partials(int32_t device, const double* mu, const double* var, int64_t M, const double* ystar, int32_t S, double* f,
                              double* dmu, double* dvar);
int32_t abo_test_acq_grad_mes(abo_gp* gp, const double* ystar, int32_t S, const double* Z, int64_t M, int32_t d, double* f, double* grad);
/* out[i] = kappa(family, d2[i]) evaluated with the device math of the kernel-matrix generator */
int32_t abo_test_kappa(int32_t device, int32_t family, const double* d2, double* out, int64_t n);
/* C[i][j] = alpha·Σ_k A[i][k]·B[j][k] + beta·C[i][j]; M, N multiples of 128, K multiple of 16,
 * leading dimensions even.  Exercises the fp64 MFMA tile core every solver stage is built on. */
int32_t abo_test_gemm_nt(int32_t device, const double* A, const double* B, double* C, int32_t M,
                         int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, double alpha,
                         double beta);
/* --- the fp64 MFMA GEMM family (csrc/gemm.hip), mode by mode ---
 * kmode: 0 = K_FULL, 1 = K_A_LOWER (tile row ti sums k < (ti+1)·128), 2 = K_A_UPPER (k ≥ ti·128), 3 = K_B_LOWER (tile column tj sums
 * k < (tj+1)·128), 4 = K_B_UPPER (k ≥ tj·128); every range clipped to K.
 * Path ids: what launch_gemm_nt ran. */
#define ABO_GEMM_PATH_TILED 0    /* gemm_nt_kernel, 2-D grid of 128×128 tiles × batch */
#define ABO_GEMM_PATH_SWIZZLED 1 /* gemm_nt_kernel, 1-D XCD-aware launch over the lower tiles of a square SYRK */
#define ABO_GEMM_PATH_SMALL 2    /* gemm_nt_small_kernel (at most 64 tiles, K a multiple of 128, C neither A nor B) */
#define ABO_GEMM_PATH_SKINNY 3   /* split-k: gemm_skinny_kernel<mrows/16> (M = 128, mrows in {16, 32, 48, 64}) */
#define ABO_GEMM_PATH_SPLITK 4   /* split-k: gemm_nt_kernel, one k chunk per grid z */
/* abo_test_gemm_nt with every field of the launcher's argument block: C[b] = alpha·A[b]·B[b]ᵀ + beta·C[b] over the k range of `kmode`,
 * Ct[b][j][i] = C[b][i][j] when Ct is given, batch b at element offsets b·sA, b·sB, b·sC, b·sCt; lower_only = 1 leaves the tiles with
 * tj > ti alone; *info != 0 (device memory, may be null) leaves everything alone.  ksplit > 0 (a multiple of 128; batch 1, beta 0, no Ct):
 * chunk z of the k range goes to the partial product C + z·sC, and a chunk outside a tile's range writes nothing; with M = 128 and mrows
 * in {16, 32, 48, 64} only the first mrows rows of A and of every partial exist.  M, N multiples of 128; K a multiple of 16 (of 128
 * under split-k); lda, ldb even.  *path = the ABO_GEMM_PATH_* that ran. */
int32_t abo_test_gemm_args(int32_t device, const double* A, const double* B, double* C, double* Ct, int64_t lda, int64_t ldb, int64_t ldc,
                           int64_t ldct, int64_t sA, int64_t sB, int64_t sC, int64_t sCt, int32_t M, int32_t N, int32_t K, int32_t kmode,
                           int32_t lower_only, int32_t batch, double alpha, double beta, int32_t ksplit, int32_t mrows, const int64_t* info,
                           int32_t* path);
/* The launcher's choice alone (no GPU needed): *path for that shape; in_place = 1: C is one of the operands.  Honours ABO_GEMM_SMALL
 * (0 never / 1 always the small kernel) and ABO_GEMM_NO_SWIZZLE as read at the time of the call. */
int32_t abo_test_gemm_path(int32_t M, int32_t N, int32_t K, int32_t kmode, int32_t lower_only, int32_t batch, int32_t ksplit,
                           int32_t mrows, int32_t in_place, int32_t* path);
/* The swizzled launch's map in its two steps (no GPU needed): workgroup L of the padded 1-D grid of ⌈tiles/8⌉·8 → position *Q in the
 * tile sequence (*Q ≥ tiles: the workgroup idles), and position Q < T(T+1)/2 → lower tile (*ti, *tj ≤ *ti) of a T×T tile grid walked in
 * super-rows of G tile rows (production: G = 4). */
int32_t abo_test_gemm_swz_q(int32_t tiles, int32_t L, int32_t* Q);
int32_t abo_test_gemm_swz_map(int32_t T, int32_t G, int32_t Q, int32_t* ti, int32_t* tj);
/* launch_qei_pass: C[z][r][j] = alpha·Σ_{k in chunk z ∩ range} A[r][k]·B[j][k], r < rows16, j < nB; row blocks of B are 64 wide and the
 * triangular range of block tj is that of the 128-row block tj/2.  ksplit = 0: one chunk.  ABO_EINVAL, and no launch, for what the
 * launcher refuses: rows16 not in {16, 32, 48, 64}, nB or K no multiple of 128, odd lda / ldb, a K_A_* kmode, ksplit no multiple of 128 */
int32_t abo_test_qei_pass(int32_t device, const double* A, int64_t lda, int32_t rows16, const double* B, int64_t ldb, int64_t nB, int32_t K,
                          double alpha, double* C, int64_t ldc, int32_t kmode, int32_t ksplit, int64_t sC);
/* launch_splitk_reduce: out[r][c] = Σ_z P[z][r][c] over exactly the chunks z that intersect the k range of column tile c/128 under
 * kmode (0, 3 or 4), in chunk order; the other chunks are not read */
int32_t abo_test_splitk_reduce(int32_t device, const double* P, int64_t ldp, int64_t sP, int32_t nz, int32_t rows, int32_t cols, int32_t K,
                               int32_t ksplit, int32_t kmode, double* out, int64_t ldo);
/* launch_var_gemm: partial[tb][j] = Σ_{i in 128-row block tb, i < nvalid} (Σ_{k ≤ i} W[i][k]·Kxz[j][k])² on the fp64 matrix pipe, for
 * a lower-triangular W.  variant 0 = the launcher's rule (Np a multiple of 256: the 256-row kernel, which reads nothing of the 16×16
 * sub-tiles above the diagonal), 1 = the 128-row kernel whatever Np (it sums k < (tb+1)·128: the whole diagonal block is read) */
int32_t abo_test_var_gemm(int32_t device, const double* W, int64_t ldw, int32_t Np, int32_t nvalid, const double* Kxz, int64_t ldk, int32_t Mc,
                          double* partial, int64_t ldp, int32_t variant);
/* --- the kernel-matrix generators (csrc/kgen_core.h, kgen_grad_core.h, kgen.hip), instantiation by instantiation ---
 * Every field of the launcher's argument block (csrc/abo_kernels.h: KgenArgs), in this fixed layout; all pointers DEVICE memory except
 * mean_vec (host, n_mean ≤ 129 entries: the prior mean per output, the first one the mean of an ordinary model; n_mean = 0: zeros).
 * Xs is ALREADY scaled by s and zero padded [Np][dp] (a gradient-enhanced model: one row per training POINT, Np pads N·pt factor
 * rows); Z are the raw candidates [M][d].  Kout, mu, alpha, res may each be null as in KgenArgs. */
typedef struct abo_test_kgen_args {
    const double* Xs; const double* Z; const double* alpha; double* Kout; double* mu;
    int64_t ldk, M, j0;
    int32_t Mc, N, Np, d, dp, family;
    double s, sigma_f2;
    const double* mean_vec;
    int32_t pt, pc, point_major, dlogell, rvalid, n_mean;
    int8_t* res; int64_t res_ld, res_plane; int32_t* res_bad;
    int32_t res_n, res_sK, res_ktg, res_kmax;
} abo_test_kgen_args;
/* launch_kgen on the null stream with exactly these fields (no decision about shape, engine or dispatch is taken by the hook);
 * ABO_EINVAL, and no launch, where launch_kgen refuses: an unknown family, a dp outside the dispatch table, planes for a shape or a
 * moduli count the fused output is not built for, a res_kmax that is no multiple of 128 or exceeds Np */
int32_t abo_test_kgen(int32_t device, const abo_test_kgen_args* args);
/* launch_kgen_deriv (csrc/kgen_deriv.hip) alone, on the null stream: the rows (f, ∂f/∂z_1 … ∂f/∂z_d) of the query points pt0 … pt0 + npts − 1
 * of Z [M][d] against the N function values of a value-only model — Xs ALREADY scaled by s and zero padded [Np][dp], alpha [Np] (may be
 * null: zeros) — into Kout [rows_pad][ldk] and mu_rows [rows_pad] (may be null); all pointers DEVICE memory.  Rows behind npts·(d + 1)
 * up to rows_pad and the columns N … Np − 1 are written as 0, nothing else is.  ABO_EINVAL, and no launch, where the launcher refuses:
 * d > 32, a dp outside 1, 2, 4, 8, 16, 32 or below d, a family other than SE / Matérn-5/2 / Matérn-7/2, Np no multiple of 128, N > Np,
 * ldk < Np, a chunk outside [0, M), rows_pad < npts·(d + 1) */
int32_t abo_test_kgen_deriv(int32_t device, const double* Xs, const double* alpha, const double* Z, double* Kout, double* mu_rows,
                            int64_t ldk, int64_t M, int64_t pt0, int32_t npts, int64_t rows_pad, int32_t N, int32_t Np, int32_t d, int32_t dp,
                            int32_t family, double s, double sigma_f2, double mean_c);
/* launch_cand_newcol (grad = 0: column `col` of a resident K_ZX, Xs row `col`) or launch_cand_newcol_grad (grad = 1: training row
 * (point pt, output q) against the function value of every candidate, written to column `col`) */
int32_t abo_test_cand_newcol(int32_t device, const double* Xs, const double* Z, double* Kzx, int64_t ld, int64_t M, int32_t col, int32_t grad,
                             int32_t pt, int32_t q, int32_t d, int32_t dp, int32_t family, double s, double sigma_f2);
/* --- the factorisation family (csrc/chol.hip and the blocked driver of csrc/api.hip), piece by piece ---
 * Every pointer is DEVICE memory; info is a device int64 the caller presets (0: run; anything else: every kernel leaves its outputs
 * alone, but for the zeroing workgroups of the panel's diagonal-block launch).  Each hook hands its arguments to the launcher(s) named,
 * on the null stream, and waits; ABO_EINVAL, and no launch, for arguments the launcher cannot take.
 * launch_chol_diag (mode 0): the 128×128 block at (r0, r0) of K [..][ld] → L in place (zeros above the diagonal), its inverse to the
 * same block of W (lower) and WT (upper, the transpose); a pivot that is no positive normal number: *info = r0 + j + 1, nothing written. */
int32_t abo_test_chol_diag(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t r0, int64_t* info);
/* launch_potf2_diag into a scratch operand stream, then (nrows > 0) launch_trsm_stream from it: the block at (r0, r0) → L, the eight
 * 16×16 diagonal sub-blocks of its inverse to W / WT, rows r0+128 … r0+128+nrows of columns r0 … r0+127 → A·L⁻ᵀ in place; zero_rows:
 * rows r0 … r0+127 of W and WT are zeroed over all ld columns outside the diagonal block.  r0, ld multiples of 128, nrows of 16. */
int32_t abo_test_chol_panel(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t r0, int32_t nrows, int32_t zero_rows,
                            int64_t* info);
/* launch_trtri_diag_batched (mode 2): the inverses of the first nblocks 128×128 diagonal blocks of a finished L, to W and WT */
int32_t abo_test_trtri_batched(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t nblocks, int64_t* info);
/* chol_blocked then trinv_blocked (what a fit runs on its kernel matrix) on the caller's K [Np][ld] with strips of sw columns,
 * super-strips of ss while at least super_rows rows remain (the library's own: 512, 1024, 6144): L → K, L⁻¹ → W, L⁻ᵀ → WT.
 * Np, ld, sw, ss multiples of 128, ss of sw.  With Np > 128 rows < Np of W / WT are zeroed by the chain; with Np = 128 only the block is
 * written. */
int32_t abo_test_chol_blocked(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t Np, int32_t sw, int32_t ss,
                              int32_t super_rows, int64_t* info);
/* launch_trmv: out[r] = Σ_k Wm[r][k]·v[k] over the triangle (lower = 1: k ≤ r, 0: r ≤ k < Np), r < Np; ld even */
int32_t abo_test_trmv(int32_t device, const double* Wm, int64_t ld, const double* v, double* out, int32_t Np, int32_t lower);
/* launch_tri_skinny (append_batch.hip): out [N][kp] = tri(Wm)·V over the triangle as abo_test_trmv, V [N][kp] and out row-major with
 * kp = k padded to a multiple of 16 (the caller pads V with zero columns), 1 ≤ k ≤ 64; only rows and columns < N of Wm are read for
 * the sum; ld a multiple of 4 and ≥ N padded to 16.  Device pointers. */
int32_t abo_test_tri_skinny(int32_t device, const double* Wm, int64_t ld, const double* V, double* out, int32_t N, int32_t k, int32_t lower);
/* the sizes (factor rows) of the live views on gp's factor storage, ascending, into out[0 … cap); *n = how many there are */
int32_t abo_test_live_views(abo_gp* gp, int64_t* out, int32_t cap, int32_t* n);
/* launch_nlml_terms: out[0] = 2·Σ_{i<N} log L[i][i], out[1] = Σ_{i<N} delta[i]·alpha[i] */
int32_t abo_test_nlml_terms(int32_t device, const double* L, int64_t ld, const double* delta, const double* alpha, int32_t N, double* out);
/* launch_append with every field of its argument block (csrc/abo_kernels.h: AppendArgs) */
typedef struct abo_test_append_args {
    double* L; double* W; double* WT;
    int64_t ld;
    const double* krow; const double* lvec; const double* vvec;
    const double* alpha_old; double* alpha_new; double* vext;
    const double* delta;
    int32_t N, cap;
    double kss;
    double* scal;
    int64_t* info;
} abo_test_append_args;
int32_t abo_test_append(int32_t device, const abo_test_append_args* args);
/* --- the selection family (csrc/misc.hip): epilogue, top-k on every route, survivor bookkeeping, streaming pieces ---
 * Every pointer is DEVICE memory unless stated otherwise.  Each hook hands its arguments to ONE launcher on the null stream and waits;
 * ABO_EINVAL, and no launch, for null pointers and for shapes the launcher cannot take.
 * Route ids: what launch_topk runs for k out of M. */
#define ABO_TOPK_PATH_NONE (-1)    /* k <= 0: nothing */
#define ABO_TOPK_PATH_SMALL 0      /* one workgroup's radix select (k <= 1024, M <= 16384) */
#define ABO_TOPK_PATH_SLICES 1     /* radix select per slice, then one merge (1 < k <= 1024) */
#define ABO_TOPK_PATH_ARGMAX 2     /* two plain reductions (k = 1, M > 16384) */
#define ABO_TOPK_PATH_BLOCKSORT 3  /* the block-sort chain; threshold rounds of 1024 for k > 1024 */
/* The launcher's choice alone (no GPU needed; out is HOST memory): out[6] = {route, kreal = min(k, max(M, 1)), SLICES: slice length and
 * pairs the merge reads, BLOCKSORT: threshold rounds and launches of the first round's sort}; zeros where a field does not apply */
int32_t abo_test_topk_plan(int64_t M, int32_t k, int64_t* out);
/* launch_topk of scores[0..M) → top_val / top_idx [k].  The hook owns the workspace: each of its four buffers has exactly
 * topk_workspace_entries(M, k) entries — what every caller in the library allocates — and a sentinel region behind them;
 * *guards_ok (HOST) = 1 when every sentinel of the four regions survived the call, 0 otherwise. */
int32_t abo_test_topk(int32_t device, const double* scores, int64_t M, int32_t k, int64_t idx_base, double* top_val, int64_t* top_idx,
                      int32_t* guards_ok);
/* launch_prune_compact: sel[0 .. *count) = the j < M, ascending, with !(ub[j] + |ub[j]|·2⁻³⁰ + abs_margin < *tau); the scan's scratch
 * is the hook's.  ABO_EINVAL, before any launch, where the launcher refuses (M <= 0, M >= 2^31). */
int32_t abo_test_prune_compact(int32_t device, const double* ub, int64_t M, const double* tau, double abs_margin, int64_t* sel, int64_t* count);
/* launch_prune_min_scatter: ub[sel[i]] = min(ub[sel[i]], ub2[i]), i < n, NaN on either side giving NaN */
int32_t abo_test_prune_min_scatter(int32_t device, double* ub, const int64_t* sel, const double* ub2, int64_t n);
/* launch_prune_map: top_idx[e] = sel[top_idx[e]] + idx_base for e < k, −1 stays */
int32_t abo_test_prune_map(int32_t device, int64_t* top_idx, int32_t k, const int64_t* sel, int64_t idx_base);
/* launch_finalize with every field of its argument block (csrc/abo_kernels.h: FinalizeArgs).  partial may be null when T = 0, mu_in
 * when head_g is given; mu_eps goes with mu_tail; by outputs (pc > 1, point_major = 0) needs Mpts > 0. */
typedef struct abo_test_finalize_args {
    const double* partial; const double* mu_in;
    double* mu_out; double* var_out; double* score_out;
    double* mu_tail; const double* mu_eps; const double* head_g; const double* ssq_g;
    int64_t ldp, j0, M, Mpts;
    double sigma_f2, p0, best_y, prior_grad;
    int32_t T, Mc, kind, pc, point_major, reserved;
} abo_test_finalize_args;
int32_t abo_test_finalize(int32_t device, const abo_test_finalize_args* args);
/* launch_cand_gemv: c[j] = Σ_{k<n} Kzx[j][k]·v[k], j < M.  ld even and >= n + 1 (rows and v are read in pairs: v holds n rounded up to
 * even entries; Kzx and v 16-byte aligned) */
int32_t abo_test_cand_gemv(int32_t device, const double* Kzx, int64_t ld, const double* v, int32_t n, int64_t M, double* c);
/* launch_downdate: mu[j] = fma(c[j], beta, mu[j]); var[j] = var[j] − c[j]·c[j]/s2, j < M */
int32_t abo_test_downdate(int32_t device, double* mu, double* var, const double* c, int64_t M, double beta, double s2);
/* launch_grad_cov with every field of its argument block (GradCovArgs) and the number of points (one workgroup each): V [npoints·p][ldv],
 * mu_rows [npoints·p]; cov_out / mu_out / score_out (each may be null) are indexed from point pt0.  ABO_EINVAL where the launcher
 * refuses (p·p + p doubles beyond the LDS of a workgroup). */
int32_t abo_test_grad_cov(int32_t device, const double* V, const double* mu_rows, int64_t ldv, int32_t R, int32_t p, int64_t pt0,
                          double prior0, double prior_g, double beta, double* cov_out, double* mu_out, double* score_out, int32_t npoints);
/* launch_gather_points: out[j][0..d) = Z[idx[j] − idx_base][0..d), zeros for idx[j] < 0, j < k */
int32_t abo_test_gather_points(int32_t device, const double* Z, const int64_t* idx, int64_t idx_base, int32_t k, int32_t d, double* out);
/* launch_pick_record: rec[3 + d] = {tv[0], (double)ti[0], mu[ti[0] − idx_base], Z[ti[0] − idx_base][0..d)}, zeros behind ti[0] < 0 */
int32_t abo_test_pick_record(int32_t device, const double* tv, const int64_t* ti, int64_t idx_base, const double* Z, const double* mu,
                             int32_t d, double* rec);
/* launch_score: score[j] = the epilogue `kind` at (mu[j], var[j]) by the plain scoring kernel — what finalize's score is held against */
int32_t abo_test_score(int32_t device, const double* mu, const double* var, double* score, int64_t M, int32_t kind, double p0, double best_y);
/* --- the int8 residue engine (csrc/ozaki.hip), stage by stage ---
 * Every pointer is DEVICE memory unless stated otherwise.  Each hook hands its arguments to ONE stage launcher (launch_oz_rowscale,
 * launch_oz_quant, launch_oz_gemm, launch_oz_crt) on the null stream and waits; ABO_EINVAL, and no launch, for what the launcher
 * cannot take.  Layouts: a residue plane is blocks of 256 rows x 64 k-bytes (oz_plane_off), U blocks of one 256 x 256 tile and
 * modulus (oz_u_block); tests/oz_ref.py packs and unpacks both.
 * Row scales: sexp[0 .. rows256) of the first nrows rows of the lower-triangular W [nrows][ldw] under the nmod-modulus plan and
 * kbits bits of K; columns k % kper != 0 weighted by 2^ktg.  delta non-null: the guard of a short plan from the g_* fields (OzGuardArgs:
 * eP and sK of the full plan, sK of the short one, kmax, the two reconstruction bounds); kper = 1 then. */
int32_t abo_test_oz_rowscale(int32_t device, const double* W, int64_t ldw, int32_t nrows, int32_t rows256, int32_t nmod, int32_t kper, int32_t ktg,
                             int32_t kbits, int32_t g_eP_full, int32_t g_sK_b, int32_t g_sK_full, double g_kmax, double g_rec_b, double g_rec_full,
                             int32_t* sexp, double* delta);
/* oz_quant_kernel with every field of OzQuantArgs but the plan (nmod in its place): out = nmod planes, `plane` bytes apart, of
 * rows_out (a multiple of 256) rows with ld bytes each, of which cols_out are written: residues of rint(in * 2^s) for r < rows_in,
 * k < cols_in (lower: k <= r), zeros elsewhere; s = srow[r] when given, else sconst; bad[r] = 1 for rows holding a value that is not
 * below 1e300 (never cleared here). */
typedef struct abo_test_oz_quant_args {
    const double* in; int64_t ldin;
    int32_t rows_in, cols_in, rows_out, cols_out, lower, sconst;
    const int32_t* srow;
    int32_t kper, ktg, rmode, rper, rtg, nmod;
    int64_t r0, rpts;
    int8_t* out; int64_t ld, plane;
    int32_t* bad;
} abo_test_oz_quant_args;
int32_t abo_test_oz_quant(int32_t device, const abo_test_oz_quant_args* args);
/* the persistent residue GEMM on given planes: KR [nmod][Mc256][Np256], WR [nmod][.][Np256] with w_plane bytes between planes (0:
 * Np256^2) -> U for the first rblocks (0: all) 256-row blocks.  PRECONDITION (not checked): WR is lower-triangular.  The tile counters
 * are the hook's, behind Mc256 flag ints as in production, zeroed once.  launches = 2: GEMM into a scratch U, a reconstruction of it
 * into a throw-away buffer (which resets the counters), and the GEMM again WITHOUT a memset, into U. */
int32_t abo_test_oz_gemm(int32_t device, const int8_t* KR, const int8_t* WR, int32_t Np256, int32_t Mc256, int32_t nmod, int32_t rblocks,
                         int64_t w_plane, int8_t* U, int32_t launches);
/* the reconstruction of U (Ti row blocks): V non-null -> V [Mc][ldv] itself (oz_crt_v_kernel), else partial [Np/128][ldp], the column
 * sums of squares per 128-row block — guarded when delta is given.  nmod 14 and 8 run the compile-time forms unless generic = 1.
 * ctr_reset (or null): 8 ints the kernel zeroes. */
int32_t abo_test_oz_crt(int32_t device, const int8_t* U, int32_t Ti, int32_t nmod, const int32_t* sexp, int32_t sK, const int32_t* bad_row,
                        const int32_t* bad_col, int32_t Np, int32_t Mc, int32_t nvalid, int32_t rmode, int32_t rper, int32_t rtg, int64_t r0,
                        int64_t rpts, const double* delta, double* partial, int64_t ldp, double* V, int64_t ldv, int32_t generic,
                        int32_t* ctr_reset);
/* the GEMM epilogue's residue arithmetic (oz_mod_pack4_mad) on quads: packed[i] = the bytes of x[4i .. 4i+3] mod the l-th modulus */
int32_t abo_test_oz_modpack(int32_t device, const int32_t* x, int64_t n4, int32_t l, int32_t* packed);
/* HOST only, no device: the tile list of a residue GEMM over Ti x Tj tiles and nmod moduli as the kernel decodes it: *count = 8 * per_list
 * (the launcher's `blocks`), tiles[y * per_list + q] = ti | tj << 9 | l << 20, or -1 for a padding block (tiles may be null) */
int32_t abo_test_oz_tickets(int32_t Ti, int32_t Tj, int32_t nmod, int32_t* tiles, int64_t* count);
/* --- the knowledge gradient's row kernel (csrc/kg.hip) on lines handed in directly, no model ---
 * launch_kg_rows on the null stream: row i < Ma has the Mb lines (intercept a[j], slope B[i·ldb + j]) and — self_a and self_b given, both
 * or neither — its own line (self_a[i], self_b[i]); val[i] = E[max_j (a_j + b_ij·Z)] − max_j a_j, nenv[i] = lines on the upper envelope
 * (0 for a row with a non-finite value, whose val is NaN).  1 <= Mb <= 8192, ldb >= Mb.  Every pointer is DEVICE memory. */
int32_t abo_test_kg_lines(int32_t device, const double* a, const double* B, int64_t ldb, int32_t Ma, int32_t Mb, const double* self_a,
                          const double* self_b, double* val, int32_t* nenv);
#endif /* ABO_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif /* ABO_HIP_H */
