// Scoring and selection of the single-device host driver: an objective's scores of M candidates from the posterior pass
// (posterior.hip), the selection of the k best — the pruned top-k (prune_plan decides, prune_select runs it) or the
// plain one over all scores —, and the entry points abo_acq, abo_acq_terms, abo_acq_mes.  Host-side orchestration only; what other
// units call is declared in abo_state.h and abo_internal.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "abo_state.h"
#include "abo_kernels.h"

using namespace abo;

namespace abo {    // declared in abo_state.h
// C-ABI terms → the kernels' form; validates kinds against the handle (GRADNORM_UCB needs gradient outputs)
int32_t make_terms(const abo_gp* g, const abo_acq_term* terms, int32_t n, AcqTerms* out, const char* fn) {
    if (!terms || n < 1) return fail(ABO_EINVAL, "%s: an objective needs at least one term", fn);
    if (n > MAX_TERMS) return fail(ABO_EINVAL, "%s: %d terms, the library takes at most %d", fn, n, MAX_TERMS);
    out->n = n;
    for (int i = 0; i < n; ++i) {
        const int k = terms[i].kind;
        if (k == ABO_ACQ_MES) return fail(ABO_EINVAL, "%s: ABO_ACQ_MES (term %d) takes a vector of samples and is no member of a weighted sum: "
                                                      "use the abo_*_mes entry points (abo_acq_mes, abo_refine_mes, …)", fn, i);
        if (k < ABO_ACQ_EI || k > ABO_ACQ_LOGEI) return fail(ABO_EINVAL, "%s: unknown acquisition kind %d (term %d)", fn, k, i);
        if (k == ABO_ACQ_GRADNORM_UCB && (!g || g->p_out < 2))
            return fail(ABO_EINVAL, "%s: GradientNormUCB (term %d) needs a gradient-enhanced model", fn, i);
        if (!(terms[i].weight == terms[i].weight)) return fail(ABO_EINVAL, "%s: weight of term %d is not a number", fn, i);
        out->kind[i] = k; out->p0[i] = terms[i].p0; out->best_y[i] = terms[i].best_y; out->w[i] = terms[i].weight;
    }
    return ABO_OK;
}
}  // namespace abo

namespace {

AcqTerms one_term(int32_t kind, double p0, double best_y) {
    AcqTerms t{};
    t.n = 1; t.kind[0] = kind; t.p0[0] = p0; t.best_y[0] = best_y; t.w[0] = 1.0;
    return t;
}

// scores of M device-resident candidates under the objective `t` into sc_d (device), queued on the handle's stream:
//   one plain term            the fused posterior + epilogue pass (what abo_acq has always run: same bits)
//   function-value terms      ONE posterior pass, then every member's epilogue on that μ, σ² (EnsembleAcq.jl:53-55)
//   MES                       the same posterior pass, then the sum over the samples per candidate (misc.hip: score_mes_kernel)
//   a GRADNORM_UCB term       the all-output posterior per point (mean[p], covariance block) in slabs, epilogue on those
//   more: the call already ran posterior passes (a pruned selection that fell back): this one is counted next to them
int32_t score_terms_device(abo_gp* g, const double* Zd, int64_t M, const AcqTerms& t, double* sc_d, bool more = false) {
    hipStream_t s = g->stream;
    if (terms_plain(t)) {
        if (t.kind[0] != ABO_ACQ_MEAN) {
            PostOpts o;
            o.more = more;
            return posterior(g, Zd, M, t.kind[0], t.p0[0], t.best_y[0], nullptr, nullptr, sc_d, o);
        }
        // −mu only: skip the contraction (scores come from the mean pass)
        HIPCHK(g->mu_all.ensure(sizeof(double) * M));
        int32_t rc = posterior(g, Zd, M, -1, 0.0, 0.0, g->mu_all.as<double>(), nullptr, nullptr);
        if (rc) return rc;
        FinalizeArgs fa{};
        fa.partial = nullptr; fa.mu_in = g->mu_all.as<double>(); fa.score_out = sc_d; fa.ldp = 0; fa.j0 = 0; fa.M = M;
        fa.T = 0; fa.Mc = (int)M; fa.kind = ABO_ACQ_MEAN; fa.sigma_f2 = g->prm.sigma_f2;
        HIPCHK(launch_finalize(fa, s));
        return ABO_OK;
    }
    if (!terms_have_gradnorm(t)) {
        HIPCHK(g->mu_all.ensure(sizeof(double) * M));
        HIPCHK(g->var_all.ensure(sizeof(double) * M));
        int32_t rc = posterior(g, Zd, M, -1, 0.0, 0.0, g->mu_all.as<double>(), g->var_all.as<double>(), nullptr);
        if (rc) return rc;
        if (terms_mes(t))
            HIPCHK(launch_score_mes(g->mu_all.as<double>(), g->var_all.as<double>(), M, t.ystar, t.n_ystar, sc_d, nullptr, nullptr, s));
        else
            HIPCHK(launch_score_terms(g->mu_all.as<double>(), g->var_all.as<double>(), sc_d, M, t, s));
        return ABO_OK;
    }
    const int P = g->p_out;
    int64_t slab = ((int64_t)64 << 20) / ((int64_t)sizeof(double) * P * P);       // ≤ 64 MiB of covariance blocks at a time
    if (slab < 1) slab = 1;
    if (slab > M) slab = M;
    HIPCHK(g->mu_all.ensure(sizeof(double) * slab * P));
    HIPCHK(g->var_all.ensure(sizeof(double) * slab * P * P));
    for (int64_t j0 = 0; j0 < M; j0 += slab) {
        const int64_t np = (M - j0) < slab ? (M - j0) : slab;
        int32_t rc = grad_eval_device(g, Zd + j0 * g->d, np, 0.0, g->mu_all.as<double>(), g->var_all.as<double>(), nullptr);
        if (rc) return rc;
        HIPCHK(launch_score_terms_grad(g->mu_all.as<double>(), g->var_all.as<double>(), sc_d + j0, np, P, t, s));
    }
    return ABO_OK;
}

}  // namespace

namespace abo {    // declared in abo_state.h
// the overrides of abo_state.h: defined here, read below (g_prune_bound_moduli: in posterior.hip), written by test_hooks.hip alone
std::atomic<int> g_prune_bound_moduli{0};
std::atomic<int> g_prune_force_rblocks{0};
std::atomic<int> g_prune_force_mode{0};
std::atomic<int> g_prune_pre_rblocks{0};
std::atomic<int64_t> g_prune_level2_min{-1};
std::atomic<int> g_prune_tail32{-1};
std::atomic<int> g_prune_head32{-1};
std::atomic<int> g_prune_reuse{-1};
}  // namespace abo

namespace {

// A switch of the pruned selection, for A/B runs: on, unless its environment variable — read once, when the switch is made — begins
// with '0'; an override ≥ 0 (a test hook's: 0 = off, else on) wins over the environment.  One function-local static per switch.
struct EnvSwitch {
    bool env_on;
    explicit EnvSwitch(const char* name) { const char* e = getenv(name); env_on = !(e && e[0] == '0'); }
    bool operator()(int override = -1) const { return override >= 0 ? override != 0 : env_on; }
};

// The mean's tail of the M-wide FIRST bound level in fp32 (kgen_tail32.hip); ABO_PRUNE_TAIL32=0 keeps the fp64 tail there.  Every other
// bound pass — the second level, a single level — has the fp64 tail either way.
bool prune_tail32() { static const EnvSwitch sw("ABO_PRUNE_TAIL32"); return sw(g_prune_tail32.load(std::memory_order_relaxed)); }

// Survivors that the threshold pass has scored are not evaluated again (prune_survivors); ABO_PRUNE_REUSE=0 runs the survivor pass on
// them as before.
bool prune_reuse() { static const EnvSwitch sw("ABO_PRUNE_REUSE"); return sw(g_prune_reuse.load(std::memory_order_relaxed)); }

// The head of that first level by the fused kernel of kgen_head32.hip — only where the fp32 tail runs, and not under an explicit moduli
// request (ABO_PRUNE_BOUND_MODULI set, or its hook): that asks for the int8 engine.  ABO_PRUNE_HEAD32=0 keeps the fp32 tail and runs the
// int8 head (generator planes, residue GEMM, reconstruction).
bool prune_head32() {
    static const EnvSwitch sw("ABO_PRUNE_HEAD32");
    return !prune_bound_moduli_asked() && sw(g_prune_head32.load(std::memory_order_relaxed));
}

// ABO_ACQ_PRUNE=0: no pruned selection; abo_test_prune_force's mode 2 is the same, as an override
bool prune_enabled() { static const EnvSwitch sw("ABO_ACQ_PRUNE"); return sw(g_prune_force_mode.load(std::memory_order_relaxed) == 2 ? 0 : -1); }

}  // namespace

namespace abo {    // declared in abo_state.h
// rows: factor rows N of the model; int8_fused: the int8-residue engine would run this call's contraction with generator-written planes
PrunePlan prune_plan(int64_t rows, int64_t M, int k, bool want_scores, int kind, double p0, int p_out, bool int8_fused, int d) {
    PrunePlan pp{false, 0, 0, 0, 0, 0};
    const int64_t tblocks = (rows + 255) / 256;
    // R = N/8, rounded to whole 256-row blocks: the bound pass then costs 1/64 of the contraction.  On the synthetic problem of the
    // benchmark R = N/8, N/4, N/2 left 4 %, 2 %, 1 % of the candidates: R = N/4 would halve a survivor pass that costs 0.04 of the
    // full one at four times a bound pass that costs 0.016 of it.
    int rb = (int)((rows / 8 + 128) / 256);
    if (rb < 1) rb = 1;
    // Two levels: how many candidates a bound removes hardly depends on R — μ decides nearly all of it — while the
    // pass's residue work grows with R (generator, reconstruction) and R² (GEMM).  So a first level of R₀ = N/32, rounded the same
    // way, runs over all M and sets the threshold, and the N/8 pass above runs only on the S₁ candidates it leaves, at S₁/M of its
    // cost: the survivor pass sees what it saw with one level.  (A narrow SINGLE level would not do: where N/8 leaves 4 % of the
    // candidates, a narrower bound leaves more, and a 4 % survivor pass already costs twice what the narrower bound saves.)  Only where
    // R₀ is fewer blocks than R — from N = 3072 on — and, under a forced R, only when the test hook asks for one.  Measured at C3:
    // 312 survivors at N/32 against 172 at N/8, the call 24.1 → 17.8 ms (N/16: 207 survivors, 18.7 ms); N = 4096: 12.6 → 11.5 ms.
    int rb0 = (int)((rows / 32 + 128) / 256);
    if (rb0 < 1) rb0 = 1;
    bool forced = false;
    int pre = 0;
    forced = g_prune_force_rblocks.load(std::memory_order_relaxed) > 0;
    if (forced) rb = g_prune_force_rblocks.load(std::memory_order_relaxed);
    pre = g_prune_pre_rblocks.load(std::memory_order_relaxed);
    if (pre > 0) rb0 = pre;              // (a forced first level that is not below rblocks: an error the callers report)
    else if (pre < 0 || forced || rb0 >= rb) rb0 = 0;
    pp.rblocks = rb;
    pp.rblocks0 = rb0;
    pp.tail32 = rb0 > 0 && prune_tail32();
    pp.head32 = pp.tail32 && prune_head32();
    pp.reuse = prune_reuse();
    pp.k0 = k > 0 ? ((int64_t)4 * k > 1024 ? (int64_t)4 * k : 1024) : 0;
    // below 4·K0 survivors the full pass on them costs less than the ≈ 16 launches of another bound pass
    pp.level2_min = 4 * pp.k0;
    if (g_prune_level2_min.load(std::memory_order_relaxed) >= 0) pp.level2_min = g_prune_level2_min.load(std::memory_order_relaxed);
    // the survivor pass costs S/M of the full pass it replaces (plus a gather of S points): it is the cheaper of the two for any
    // S < M, and is taken while it saves at least an eighth of the pass — far more than the extra launches cost
    pp.max_survivors = M - M / 8;
    const bool monotone = kind == ABO_ACQ_EI || kind == ABO_ACQ_LOGEI || (kind == ABO_ACQ_UCB && p0 >= 0.0);
    // two passes pay from a few times the K0 exactly evaluated candidates on (M ≥ 4·K0: the threshold pass is at most a quarter of
    // what the selection can save); the compaction counts in ints and gathers with 32-bit element indices
    pp.eligible = prune_enabled() && k > 0 && !want_scores && monotone && p_out == 1 && int8_fused && rb < tblocks &&
                  M >= 4 * pp.k0 && M * (int64_t)d < ((int64_t)1 << 31);
    return pp;
}
}  // namespace abo

namespace {

// ---- the pruned selection, stage by stage -----------------------------------------------------------------------------------
// What the stages of one call share.  The device state is the handle's: pr_ub the bounds of all M candidates, pr_sel the survivor
// list, pr_tv the K0 threshold values with three words behind them — {survivor count, −Inf (test hook), the reuse's "not found" flag}.
struct PruneCall {
    abo_gp* g;
    const double* Zd;           // the M candidates, device
    int64_t M;
    int kind;                   // the one plain term
    double p0, best_y;
    const PrunePlan& pp;
    int32_t k;
    TopkWork w;
    hipStream_t s() const { return g->stream; }
    double* ub() const { return g->pr_ub.as<double>(); }
    int64_t* count_d() const { return reinterpret_cast<int64_t*>(g->pr_tv.as<double>() + pp.k0); }
    bool two_levels() const { return pp.rblocks0 > 0; }
    double abs_slack() const { return kind == ABO_ACQ_LOGEI ? PRUNE_ABS_LOGEI : PRUNE_ABS; }
};

// 1. bound pass: the chunk pipeline on the first row blocks of W — those of the first level where the plan has one.
// *available = false: the engine cannot run it after all, nothing was launched.
int32_t prune_bound(const PruneCall& c, bool* available) {
    abo_gp* g = c.g;
    *available = false;
    HIPCHK(hipEventRecord(g->evs()[EV_BOUND_BEGIN], c.s()));
    // (a first level's looser mean costs survivors alone, and the second level is there when they are many; a single level has no such net)
    PostOpts bound;
    bound.rblocks = c.two_levels() ? c.pp.rblocks0 : c.pp.rblocks; bound.tail32 = c.pp.tail32; bound.head32 = c.pp.head32;
    const int32_t rc = posterior(g, c.Zd, c.M, c.kind, c.p0, c.best_y, nullptr, nullptr, c.ub(), bound);
    if (rc == PRUNE_UNAVAILABLE) return ABO_OK;
    if (rc) return rc;
    g->pst.bound_rows = g->passes.back().rows;
    g->pst.k0 = c.pp.k0;
    HIPCHK(hipEventRecord(g->evs()[EV_BOUND_END], c.s()));
    *available = true;
    return ABO_OK;
}

// 2. threshold: exact scores of the K0 best by bound (NaN bounds first, as everywhere), τ = the k-th best of them (device, *tau)
int32_t prune_threshold(const PruneCall& c, const double** tau) {
    abo_gp* g = c.g;
    hipStream_t s = c.s();
    const int64_t K0 = c.pp.k0;
    HIPCHK(launch_topk(c.ub(), c.M, (int)K0, 0, c.w, g->pr_tv.as<double>(), g->pr_ti.as<int64_t>(), s));
    HIPCHK(launch_gather_points(c.Zd, g->pr_ti.as<int64_t>(), 0, (int)K0, g->d, g->pr_z.as<double>(), s));
    PostOpts further;
    further.more = true;
    const int32_t rc = posterior(g, g->pr_z.as<double>(), K0, c.kind, c.p0, c.best_y, nullptr, nullptr, g->pr_sc.as<double>(), further);
    if (rc) return rc;
    // (the selection below overwrites pr_ti: the candidates that pr_sc's scores belong to are kept for prune_survivors)
    if (c.pp.reuse) HIPCHK(hipMemcpyAsync(g->pr_ti0.p, g->pr_ti.p, sizeof(int64_t) * K0, hipMemcpyDeviceToDevice, s));
    HIPCHK(launch_topk(g->pr_sc.as<double>(), K0, c.k, 0, c.w, g->pr_tv.as<double>(), g->pr_ti.as<int64_t>(), s));
    *tau = g->pr_tv.as<double>() + (c.k - 1);
    if (g_prune_force_mode.load(std::memory_order_relaxed) == 1) {
        static const double ninf = -HUGE_VAL;
        HIPCHK(hipMemcpyAsync(c.count_d() + 1, &ninf, sizeof(double), hipMemcpyHostToDevice, s));
        *tau = reinterpret_cast<const double*>(c.count_d() + 1);
    }
    return ABO_OK;
}

// 3. survivors: every candidate whose guarded bound reaches τ (the k that set τ among them), in index order — and the call's one
// read-back: *S survivors; *try_reuse: the lookup of prune_survivors ran, *not_found: it missed a survivor.
int32_t prune_compact(const PruneCall& c, const double* tau, bool* try_reuse, int64_t* S, bool* not_found) {
    abo_gp* g = c.g;
    hipStream_t s = c.s();
    const int64_t K0 = c.pp.k0;
    int64_t* count_d = c.count_d();
    HIPCHK(launch_prune_compact(c.ub(), c.M, tau, c.abs_slack(), g->pr_blk.as<int>(), g->pr_sel.as<int64_t>(), count_d, s));
    HIPCHK(hipEventRecord(g->evs()[EV_THRESHOLD_END], s));
    // (the lookup of prune_survivors, ahead of the count's way to the host: the kernel reads the count itself and does nothing for more
    // than K0 survivors, and its "not found" flag comes back with the count — no synchronisation of its own)
    *try_reuse = c.pp.reuse && 2 * K0 <= PRUNE_REUSE_SLOTS;
    if (*try_reuse) {
        HIPCHK(hipMemsetAsync(count_d + 2, 0, sizeof(int64_t), s));
        HIPCHK(launch_prune_reuse_scores(g->pr_sel.as<int64_t>(), count_d, g->pr_ti0.as<int64_t>(), g->pr_sc.as<double>(), K0,
                                         g->pr_sc.as<double>() + K0, count_d + 2, s));
    }
    int64_t back[3] = {0, 0, 0};          // survivor count, (the hook's threshold), not found
    HIPCHK(hipMemcpyAsync(back, count_d, sizeof(int64_t) * (*try_reuse ? 3 : 1), hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    *S = back[0];
    *not_found = back[2] != 0;
    return ABO_OK;
}

// 3b. second level: the bound pass at rblocks on the first level's *S survivors, against the SAME τ (the k-th best exact score of any
// subset is a valid threshold).  ub keeps min(level 1, level 2) — still an upper bound for every one of the M candidates — and is
// compacted again over all M (8 bytes a candidate: cheaper than a second index map), so the list stays in index order.
int32_t prune_second_level(const PruneCall& c, const double* tau, int64_t* S) {
    abo_gp* g = c.g;
    hipStream_t s = c.s();
    HIPCHK(hipEventRecord(g->evs()[EV_BOUND2_BEGIN], s));
    HIPCHK(g->pr_z.ensure(sizeof(double) * *S * g->d));
    HIPCHK(g->pr_ub2.ensure(sizeof(double) * *S));
    HIPCHK(launch_gather_points(c.Zd, g->pr_sel.as<int64_t>(), 0, (int)*S, g->d, g->pr_z.as<double>(), s));
    PostOpts bound2;
    bound2.rblocks = c.pp.rblocks; bound2.more = true; bound2.level2 = true;
    const int32_t rc = posterior(g, g->pr_z.as<double>(), *S, c.kind, c.p0, c.best_y, nullptr, nullptr, g->pr_ub2.as<double>(), bound2);
    if (rc == PRUNE_UNAVAILABLE) return ABO_OK;          // (no scratch for the engine at this size: the first level's list goes on as it is)
    if (rc) return rc;
    g->plv.rows2 = g->passes.back().rows;
    HIPCHK(launch_prune_min_scatter(c.ub(), g->pr_sel.as<int64_t>(), g->pr_ub2.as<double>(), *S, s));
    HIPCHK(launch_prune_compact(c.ub(), c.M, tau, c.abs_slack(), g->pr_blk.as<int>(), g->pr_sel.as<int64_t>(), c.count_d(), s));
    HIPCHK(hipEventRecord(g->evs()[EV_BOUND2_END], s));
    HIPCHK(hipMemcpyAsync(S, c.count_d(), sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    g->plv.s2 = *S;
    return ABO_OK;
}

// 4. exact scores of the S survivors, in list order, and the k best of them into tv / ti (list positions).  reuse: the scores the
// threshold pass left behind its own in pr_sc are taken; else the survivor pass runs.
// With no second level and S ≤ K0 the threshold pass has scored nearly always all of them: a survivor kept because its bound reaches τ
// ranks, by bound, ahead of every candidate that does not, so were it outside the K0 best by bound, all K0 of them would survive too,
// S ≥ K0 + 1; NaN bounds are kept and rank first.  The exception is a stored bound of −Inf (LogEI where the bound's variance is ≤ 1e-12
// and Δ ≤ 0): its guard is −Inf + Inf = NaN, so it is kept, yet it ranks LAST by bound and need not be among the K0.  So the argument is
// not relied on: the lookup of prune_compact reports every survivor it did not find, and such a call runs the survivor pass as before.
// An exact score does not depend on the batch a candidate is evaluated in, so a score that was found is the bits a pass
// over the survivors would give.  (After a second level the list is a subset of the first level's, whose lookup is void: the survivor
// pass runs.)
int32_t prune_survivors(const PruneCall& c, bool reuse, int64_t S, double* tv, int64_t* ti) {
    abo_gp* g = c.g;
    hipStream_t s = c.s();
    if (reuse) {
        double* sc0 = g->pr_sc.as<double>();           // K0 scores in the order of pr_ti0; the survivors' behind them
        PHASE_EVENT(g->evs()[EV_ACQ_SCORED], s);
        HIPCHK(launch_topk(sc0 + c.pp.k0, S, c.k, 0, c.w, tv, ti, s));
        g->pr_reused = true;
        // The call's work figures (var_gemm_flop, oz_gemm_ops) stay those of the selection as an algorithm — bound pass, K0 threshold
        // candidates, S survivors — as tests/test_gpu_kgen_head32.py holds them: a pass of no chunks stands for the survivors.  No time
        // is booked against it, so a rate taken from these figures (the benchmark's residue-GEMM rate among them) credits a reusing
        // call with S/(K0 + S) of exact evaluations it did not launch (DESIGN §3b-1 says so where it gives the figures).
        g->passes.push_back({g->passes.back().chunk0 + g->passes.back().nchunk, 0, S, g->N, g->oz_plan.n, false});
        return ABO_OK;
    }
    HIPCHK(g->pr_z.ensure(sizeof(double) * S * g->d));
    HIPCHK(g->pr_sc.ensure(sizeof(double) * S));
    HIPCHK(launch_gather_points(c.Zd, g->pr_sel.as<int64_t>(), 0, (int)S, g->d, g->pr_z.as<double>(), s));
    PostOpts further;
    further.more = true;
    const int32_t rc = posterior(g, g->pr_z.as<double>(), S, c.kind, c.p0, c.best_y, nullptr, nullptr, g->pr_sc.as<double>(), further);
    if (rc) return rc;
    PHASE_EVENT(g->evs()[EV_ACQ_SCORED], s);
    // the selection among the exactly evaluated: list positions are in index order, so ties fall as they do over all M
    HIPCHK(launch_topk(g->pr_sc.as<double>(), S, c.k, 0, c.w, tv, ti, s));
    return ABO_OK;
}

// The pruned selection on device candidates Zd.  *done = false: nothing selected (the engine was not available after all, or too many
// candidates survived) — the caller runs the ordinary pass, with more = true when passes were launched here.
int32_t prune_select(abo_gp* g, const double* Zd, int64_t M, const AcqTerms& t, const PrunePlan& pp, int64_t idx_base, int32_t k,
                     TopkWork w, double* tv, int64_t* ti, bool* done) {
    const PruneCall c{g, Zd, M, t.kind[0], t.p0[0], t.best_y[0], pp, k, w};
    const int64_t K0 = pp.k0;
    *done = false;
    const int64_t nb = (M + PRUNE_SCAN_E - 1) / PRUNE_SCAN_E;
    HIPCHK(g->pr_ub.ensure(sizeof(double) * M));
    HIPCHK(g->pr_z.ensure(sizeof(double) * K0 * g->d));
    HIPCHK(g->pr_sc.ensure(sizeof(double) * 2 * K0));            // the threshold pass's scores, then those of ≤ K0 survivors taken from them
    HIPCHK(g->pr_sel.ensure(sizeof(int64_t) * M));
    HIPCHK(g->pr_blk.ensure(sizeof(int) * nb + 16));
    HIPCHK(g->pr_tv.ensure(sizeof(double) * (K0 + 3)));          // K0 values, then the three words of PruneCall::count_d
    HIPCHK(g->pr_ti.ensure(sizeof(int64_t) * K0));
    HIPCHK(g->pr_ti0.ensure(sizeof(int64_t) * K0));              // the threshold pass's K0 candidates
    g->pr_reused = false;
    HIPCHK(g->events(EV_BASE));          // (the slots of this call by index, never by pointer: the passes below may grow, and move, the context's event list)

    bool available = false;
    int32_t rc = prune_bound(c, &available);
    if (rc || !available) return rc;
    const double* tau = nullptr;
    if ((rc = prune_threshold(c, &tau))) return rc;
    bool try_reuse = false, not_found = false;
    int64_t S = 0;
    if ((rc = prune_compact(c, tau, &try_reuse, &S, &not_found))) return rc;
    if (c.two_levels()) {
        g->plv.rows1 = g->pst.bound_rows;
        g->plv.s1 = S;
        if (S > pp.level2_min && (rc = prune_second_level(c, tau, &S))) return rc;
    }
    g->pst.survivors = S;
    if (S < k || S > pp.max_survivors) { g->pst.fallback = 1; return ABO_OK; }
    const bool reuse = try_reuse && g->plv.rows2 == 0 && S <= K0 && !not_found;
    if ((rc = prune_survivors(c, reuse, S, tv, ti))) return rc;
    HIPCHK(launch_prune_map(ti, k, g->pr_sel.as<int64_t>(), idx_base, c.s()));
    HIPCHK(hipEventRecord(g->evs()[EV_SURVIVORS_END], c.s()));
    g->pst.pruned = 1;
    *done = true;
    return ABO_OK;
}

}  // namespace

namespace abo {    // declared in abo_state.h
int32_t acq_terms_impl(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, const AcqTerms& t, int64_t idx_base,
                       double* scores, int32_t out_space, int32_t k, double* top_val, int64_t* top_idx, int32_t top_space) {
    if (M < 0 || (M > 0 && !Z)) return fail(ABO_EINVAL, "abo_acq: bad candidate buffer");
    if (k < 0) return fail(ABO_EINVAL, "abo_acq: k = %d is negative", k);
    if (k > 0 && (!top_val || !top_idx)) return fail(ABO_EINVAL, "abo_acq: k > 0 needs top_val and top_idx");
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    double* sc_d = nullptr;
    PinStage pin(g->ctx);
    const bool with_var = !(terms_plain(t) && t.kind[0] == ABO_ACQ_MEAN);
    const bool fused_timings = !terms_have_gradnorm(t);           // the slab path does not keep per-chunk events
    g->pst = abo_prune_stats{};
    g->plv = abo_gp::PruneLevels{};
    g->pr_reused = false;
    PrunePlan pp{false, 0, 0, 0, 0, 0};
    if (M > 0 && terms_plain(t)) {
        int nm = 0;
        const bool int8_fused = wants_int8(g, true, 1, &nm) && kgen_writes_residues(kgen_model_args(g, false), nm);
        pp = prune_plan(g->N, M, k, scores != nullptr, t.kind[0], t.p0[0], g->p_out, int8_fused, g->d);
        if (pp.eligible && pp.rblocks0 >= pp.rblocks)          // (abo_test_prune_levels alone can ask for this)
            return fail(ABO_EINVAL, "abo_acq: a first bound level of %d row blocks is not below the bound pass's %d", pp.rblocks0, pp.rblocks);
    }
    TopkWork w{};
    double* tv = top_val;
    int64_t* ti = top_idx;
    if (k > 0) {
        const int64_t we = topk_workspace_entries(M, pp.eligible && pp.k0 > k ? (int)pp.k0 : k);
        HIPCHK(g->tk_keys0.ensure(sizeof(uint64_t) * we));
        HIPCHK(g->tk_keys1.ensure(sizeof(uint64_t) * we));
        HIPCHK(g->tk_idx0.ensure(sizeof(int64_t) * we));
        HIPCHK(g->tk_idx1.ensure(sizeof(int64_t) * we));
        w = TopkWork{{g->tk_keys0.as<uint64_t>(), g->tk_keys1.as<uint64_t>()}, {g->tk_idx0.as<int64_t>(), g->tk_idx1.as<int64_t>()}};
        if (top_space == ABO_HOST) {
            HIPCHK(g->top_val.ensure(sizeof(double) * k));
            HIPCHK(g->top_idx.ensure(sizeof(int64_t) * k));
            tv = g->top_val.as<double>();
            ti = g->top_idx.as<int64_t>();
        }
    }
    bool selected = false;
    if (M > 0) {
        const double* Zd = nullptr;
        int32_t rc = stage_candidates(g, Z, M, z_space, &Zd);
        if (rc) return rc;
        HIPCHK(hipEventRecord(g->evs()[EV_ACQ_BEGIN], s));
        if (pp.eligible) {
            rc = prune_select(g, Zd, M, t, pp, idx_base, k, w, tv, ti, &selected);
            if (rc) return rc;
        }
        if (!selected) {
            if (scores && out_space == ABO_DEVICE) sc_d = scores;
            else { HIPCHK(g->score_all.ensure(sizeof(double) * M)); sc_d = g->score_all.as<double>(); }
            rc = score_terms_device(g, Zd, M, t, sc_d, /*more=*/g->pst.bound_rows > 0);
            if (rc) return rc;
            PHASE_EVENT(g->evs()[EV_ACQ_SCORED], s);
        }
    } else {
        HIPCHK(hipEventRecord(g->evs()[EV_ACQ_BEGIN], s));
        PHASE_EVENT(g->evs()[EV_ACQ_SCORED], s);
    }
    if (k > 0) {
        if (!selected) HIPCHK(launch_topk(sc_d, M, k, idx_base, w, tv, ti, s));
        if (top_space == ABO_HOST) {
            HIPCHK(pin.d2h(top_val, tv, sizeof(double) * k, s));             // through the pinned block, copied on after the sync
            HIPCHK(pin.d2h(top_idx, ti, sizeof(int64_t) * k, s));
        }
    }
    HIPCHK(hipEventRecord(g->evs()[EV_ACQ_END], s));
    if (scores && out_space == ABO_HOST && M > 0) {
        int32_t rc = copy_out(scores, sc_d, sizeof(double) * M, ABO_HOST, s);
        if (rc) return rc;
    }
    HIPCHK(wait_stream(s));
    pin.flush();
    if (M > 0 && fused_timings) collect_posterior_timings(g, with_var);
    std::vector<hipEvent_t>& ev = g->evs();
    g->tm.acq_topk_ms = phase_events() ? ev_ms(ev[EV_ACQ_SCORED], ev[EV_ACQ_END]) : 0.0;
    g->tm.acq_total_ms = ev_ms(ev[EV_ACQ_BEGIN], ev[EV_ACQ_END]);
    if (g->pst.bound_rows > 0) {
        const bool l2 = g->plv.rows2 > 0;
        if (g->plv.rows1 > 0) g->plv.ms1 = ev_ms(ev[EV_BOUND_BEGIN], ev[EV_BOUND_END]);
        if (l2) g->plv.ms2 = ev_ms(ev[EV_BOUND2_BEGIN], ev[EV_BOUND2_END]);
        g->pst.bound_ms = ev_ms(ev[EV_BOUND_BEGIN], ev[EV_BOUND_END]) + g->plv.ms2;
        g->pst.threshold_ms = ev_ms(ev[EV_BOUND_END], ev[EV_THRESHOLD_END]);
        // (the survivor pass begins where the last compaction ended: the second level's, where it ran)
        g->pst.survivor_ms = g->pst.pruned ? ev_ms(ev[l2 ? EV_BOUND2_END : EV_THRESHOLD_END], ev[EV_SURVIVORS_END]) : 0.0;
    }
    return ABO_OK;
}
}  // namespace abo

// abo_acq with separate memory spaces for the M scores and for the k selected pairs (the multi-device driver keeps the
// pairs on the device for the RCCL exchange while the scores, when asked for, go to the caller's host array)
int32_t abo::acq_ex(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, int32_t kind, double p0,
                    double best_y, int64_t idx_base, double* scores, int32_t out_space, int32_t k, double* top_val,
                    int64_t* top_idx, int32_t top_space) {
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (kind == ABO_ACQ_MES) return fail(ABO_EINVAL, "abo_acq: ABO_ACQ_MES takes a vector of samples: use abo_acq_mes");
    if (!plain_kind(kind)) return fail(ABO_EINVAL, "abo_acq: unknown acquisition kind %d", kind);
    return acq_terms_impl(g, Z, M, d, z_space, one_term(kind, p0, best_y), idx_base, scores, out_space, k, top_val, top_idx, top_space);
}

int32_t abo::acq_terms_ex(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, const abo_acq_term* terms, int32_t nterms,
                          int64_t idx_base, double* scores, int32_t out_space, int32_t k, double* top_val, int64_t* top_idx,
                          int32_t top_space) {
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    AcqTerms t{};
    rc = make_terms(g, terms, nterms, &t, "abo_acq_terms");
    if (rc) return rc;
    return acq_terms_impl(g, Z, M, d, z_space, t, idx_base, scores, out_space, k, top_val, top_idx, top_space);
}

extern "C" {

int32_t abo_acq(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, int32_t kind, double p0,
                double best_y, int64_t idx_base, double* scores, int32_t k, double* top_val, int64_t* top_idx,
                int32_t out_space) {
    return abo::acq_ex(g, Z, M, d, z_space, kind, p0, best_y, idx_base, scores, out_space, k, top_val, top_idx, out_space);
}

int32_t abo_acq_terms(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, const abo_acq_term* terms,
                      int32_t nterms, int64_t idx_base, double* scores, int32_t k, double* top_val, int64_t* top_idx,
                      int32_t out_space) {
    return abo::acq_terms_ex(g, Z, M, d, z_space, terms, nterms, idx_base, scores, out_space, k, top_val, top_idx, out_space);
}

// max-value entropy search (the checks and the objective: api.hip) through the same stages — never the pruned selection:
// terms_plain is false
int32_t abo_acq_mes(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, const double* ystar, int32_t S, int32_t ys_space,
                    int64_t idx_base, double* scores, int32_t k, double* top_val, int64_t* top_idx, int32_t out_space) {
    int32_t rc = mes_check_samples(ystar, S, ys_space, "abo_acq_mes");
    if (rc) return rc;
    rc = check_fitted(g, d);
    if (rc) return rc;
    rc = mes_check_handle(g, "abo_acq_mes");
    if (rc) return rc;
    AcqTerms t;
    rc = mes_terms(g, ystar, S, ys_space, &t);
    if (rc) return rc;
    return acq_terms_impl(g, Z, M, d, z_space, t, idx_base, scores, out_space, k, top_val, top_idx, out_space);
}

}  // extern "C"
