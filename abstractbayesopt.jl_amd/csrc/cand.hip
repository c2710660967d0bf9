// Resident candidate sets of the single-device host driver (C5: greedy q-EI on a fixed grid with O(N·M) down-dates): a set's points
// and posterior in HBM — refresh, the rank-1 down-date behind an append, scoring and selection over the stored (μ, σ²), save /
// restore / get / exclude — and what paths.hip, qei_mc.hip and mgpu.hip read of a set (abo_internal.h).  The set's block-form q-EI
// state is driven by qei_host.hip.  Host-side orchestration only; the struct and what crosses a unit boundary are in abo_state.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <new>

#include "abo_state.h"

using namespace abo;

int32_t abo::cand_topk(abo_gp* g, abo_cand* c, const double* sc_d, int32_t k, int64_t idx_base, double* top_val, int64_t* top_idx, int32_t out_space) {
    hipStream_t s = g->stream;
    const int64_t we = topk_workspace_entries(c->M, k);
    HIPCHK(c->tk_keys0.ensure(sizeof(uint64_t) * we));
    HIPCHK(c->tk_keys1.ensure(sizeof(uint64_t) * we));
    HIPCHK(c->tk_idx0.ensure(sizeof(int64_t) * we));
    HIPCHK(c->tk_idx1.ensure(sizeof(int64_t) * we));
    TopkWork w{{c->tk_keys0.as<uint64_t>(), c->tk_keys1.as<uint64_t>()}, {c->tk_idx0.as<int64_t>(), c->tk_idx1.as<int64_t>()}};
    double* tv = top_val;
    int64_t* ti = top_idx;
    if (out_space == ABO_HOST) {
        HIPCHK(c->top_val.ensure(sizeof(double) * k));
        HIPCHK(c->top_idx.ensure(sizeof(int64_t) * k));
        tv = c->top_val.as<double>();
        ti = c->top_idx.as<int64_t>();
    }
    HIPCHK(launch_topk(sc_d, c->M, k, idx_base, w, tv, ti, s));
    if (out_space == ABO_HOST) {
        int32_t rc = copy_out(top_val, tv, sizeof(double) * k, ABO_HOST, s); if (rc) return rc;
        rc = copy_out(top_idx, ti, sizeof(int64_t) * k, ABO_HOST, s); if (rc) return rc;
    }
    return ABO_OK;
}

// The tail every scoring call over the stored (μ, σ²) shares: the scores go to the caller's device array or to the set's own, `score`
// launches them, the k best are selected (top_space), host scores are copied out, and the call waits for its stream.
static int32_t score_select(abo_gp* g, abo_cand* c, const std::function<hipError_t(double*, hipStream_t)>& score, int64_t idx_base,
                            double* scores, int32_t out_space, int32_t k, double* top_val, int64_t* top_idx, int32_t top_space) {
    hipStream_t s = g->stream;
    double* sc_d = (scores && out_space == ABO_DEVICE) ? scores : nullptr;
    if (!sc_d) { HIPCHK(c->score.ensure(sizeof(double) * (c->M > 0 ? c->M : 1))); sc_d = c->score.as<double>(); }
    HIPCHK(score(sc_d, s));
    if (k > 0) { int32_t rc = cand_topk(g, c, sc_d, k, idx_base, top_val, top_idx, top_space); if (rc) return rc; }
    if (scores && out_space == ABO_HOST && c->M > 0) {
        int32_t rc = copy_out(scores, sc_d, sizeof(double) * c->M, ABO_HOST, s);
        if (rc) return rc;
    }
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

// The down-date column c(z) = Σ_{k ≤ Rq} k(z, x_k)·vext[k] of appended row Rq from kernel values, for a set without a resident K_ZX:
// 65 536 candidates per launch, the rows up to the appended one.  P = rows per append.  P > 1 (a gradient-enhanced model): all points,
// pt = P outputs each, of which the first Rq + 1 rows are valid — a partly appended point.  P = 1: one output per point, so simply
// Rq + 1 points; rvalid stays 0 (it is read for pt > 1 only) and pt = 1 is what kgen_model_args gives for the standard GP a one-row
// append belongs to — abo_cand_downdate and cand_downdate_column fill the same arguments.
static int32_t column_from_kernel_values(abo_gp* g, abo_cand* c, const double* vext, int64_t Rq, int P, double* out) {
    const int64_t step = 65536;
    for (int64_t j0 = 0; j0 < c->M; j0 += step) {
        const int64_t m = (c->M - j0) < step ? (c->M - j0) : step;
        KgenArgs ka = kgen_model_args(g, false);
        ka.pt = P;
        ka.Z = c->Z.as<double>(); ka.alpha = vext; ka.mu = out + j0; ka.M = c->M; ka.j0 = j0; ka.Mc = (int)pad_up(m, 16);
        ka.Np = (int)pad_up(Rq + 1, TB);
        if (P > 1) ka.rvalid = (int)(Rq + 1);
        else ka.N = (int)(Rq + 1);
        HIPCHK(launch_kgen(ka, g->stream));
    }
    return ABO_OK;
}

int32_t abo::cand_acq_ex(abo_gp* g, abo_cand* c, int32_t kind, double p0, double best_y, int64_t idx_base, double* scores,
                         int32_t out_space, int32_t k, double* top_val, int64_t* top_idx, int32_t top_space) {
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_acq: null argument");
    if (kind == ABO_ACQ_MES) return fail(ABO_EINVAL, "abo_cand_acq: ABO_ACQ_MES takes a vector of samples: use abo_cand_acq_mes");
    if (!plain_kind(kind)) return fail(ABO_EINVAL, "abo_cand_acq: unknown acquisition kind %d", kind);
    if (k < 0) return fail(ABO_EINVAL, "abo_cand_acq: k = %d is negative", k);
    if (k > 0 && (!top_val || !top_idx)) return fail(ABO_EINVAL, "abo_cand_acq: k > 0 needs top_val and top_idx");
    if (g->prm.device != c->device) return fail(ABO_EINVAL, "candidate set lives on device %d, model on %d", c->device, g->prm.device);
    HIPCHK(hipSetDevice(g->prm.device));
    return score_select(g, c, [&](double* sc_d, hipStream_t s) {
        return launch_score(c->mu.as<double>(), c->var.as<double>(), sc_d, c->M, kind, p0, best_y, s);
    }, idx_base, scores, out_space, k, top_val, top_idx, top_space);
}

extern "C" {

int32_t abo_cand_refresh(abo_gp* g, abo_cand* c) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    if (!c) return fail(ABO_EINVAL, "abo_cand_refresh: null candidate set");
    int32_t rc = check_fitted(g, c->d);
    if (rc) return rc;
    if (g->prm.device != c->device) return fail(ABO_EINVAL, "candidate set lives on device %d, model on %d", c->device, g->prm.device);
    HIPCHK(hipSetDevice(g->prm.device));
    if (c->M > 0) {
        // keep K_ZX resident when it fits the budget
        const char* lim = getenv("ABO_CAND_KZX_GIB");
        const double budget = (lim ? atof(lim) : 64.0) * 1073741824.0;
        const int64_t rows = pad_up(c->M, TB), ldz = g->st->cap;
        const double need = (double)rows * (double)ldz * sizeof(double);
        c->kzx_ld = 0;
        if (need <= budget) {
            const void* before = c->Kzx.p;
            const hipError_t e = c->Kzx.ensure((size_t)need);
            if (e == hipSuccess) {
                // columns ≥ Np are never written by the refresh: zero a new allocation once (later appends fill them)
                if (c->Kzx.p != before) HIPCHK(hipMemsetAsync(c->Kzx.p, 0, c->Kzx.cap, g->stream));
                c->kzx_ld = ldz;
            } else {
                (void)hipGetLastError();              // does not fit next to the model: fall back to recomputation
            }
        } else {
            c->Kzx.release();
        }
        HIPCHK(hipEventRecord(g->evs()[EV_ACQ_BEGIN], g->stream));
        PostOpts keep;
        keep.kstore = c->kzx_ld ? c->Kzx.as<double>() : nullptr; keep.ldstore = c->kzx_ld;
        rc = posterior(g, c->Z.as<double>(), c->M, -1, 0.0, 0.0, c->mu.as<double>(), c->var.as<double>(), nullptr, keep);
        if (rc) return rc;
        HIPCHK(hipEventRecord(g->evs()[EV_ACQ_SCORED], g->stream));
        HIPCHK(wait_stream(g->stream));
        collect_posterior_timings(g, true);
        g->tm.acq_topk_ms = 0.0;
        g->tm.acq_total_ms = ev_ms(g->evs()[EV_ACQ_BEGIN], g->evs()[EV_ACQ_SCORED]);
    }
    c->synced_gen = g->st->gen;
    c->synced_N = g->N;
    c->qei = abo_cand::Qei();                             // blocks and chain of an earlier q-EI batch belong to the old posterior
    return ABO_OK;
}

int32_t abo_cand_create(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, abo_cand** out) {
    if (!out) return fail(ABO_EINVAL, "abo_cand_create: null argument");
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (M < 0 || (M > 0 && !Z)) return fail(ABO_EINVAL, "abo_cand_create: bad candidate buffer");
    HIPCHK(hipSetDevice(g->prm.device));
    abo_cand* c = new (std::nothrow) abo_cand();
    if (!c) return fail(ABO_ENOMEM, "abo_cand_create: host allocation failed");
    c->set_device(g->prm.device);
    c->d = d; c->M = M;
    hipError_t e = c->Z.ensure(sizeof(double) * (M > 0 ? M : 1) * d);
    if (e == hipSuccess) e = c->mu.ensure(sizeof(double) * (M > 0 ? M : 1));
    if (e == hipSuccess) e = c->var.ensure(sizeof(double) * (M > 0 ? M : 1));
    if (e != hipSuccess) { c->free_all(); delete c; return fail(ABO_ENOMEM, "abo_cand_create: %s", hipGetErrorString(e)); }
    rc = copy_in(c->Z.p, Z, sizeof(double) * M * d, z_space, g->stream);
    if (!rc) rc = abo_cand_refresh(g, c);
    if (rc) { (void)wait_stream(g->stream); c->free_all(); delete c; return rc; }
    *out = c;
    return ABO_OK;
}

int32_t abo_cand_destroy(abo_cand* c) {
    if (!c || abo::exiting()) return ABO_OK;
    if (abo::gone(hipSetDevice(c->device))) { abo::set_exiting(); return ABO_OK; }
    c->free_all();
    delete c;
    return ABO_OK;
}

int32_t abo_cand_downdate(abo_gp* g, abo_cand* c) {
    if (!c) return fail(ABO_EINVAL, "abo_cand_downdate: null candidate set");
    int32_t rc = check_fitted(g, c->d);
    if (rc) return rc;
    const int P = g->p_out;                                // rows the append added: 1, or p for a gradient-enhanced model
    if (!g->from_append || g->st->gen != c->synced_gen || g->N != c->synced_N + P)
        return fail(ABO_EINVAL, "abo_cand_downdate: the model is not the one-point append of the model this candidate set "
                                "was last evaluated with (call abo_cand_refresh)");
    // a view that abo_append_batch made in a blocked step is an appended view WITHOUT a down-date vector (and without the one appended
    // point): whatever the set was last synced with — a view of N − 1 rows on the same storage that has since been destroyed passes
    // the test above — there is no rank-one column to apply
    if (!g->vext.p || (P == 1 && (int)g->ap_x.size() != g->d))
        return fail(ABO_EINVAL, "abo_cand_downdate: the model was made by a blocked batch append (abo_append_batch, k >= 2), which leaves "
                                "no one-point down-date (call abo_cand_refresh)");
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    if (c->M > 0) {
        // c(z) = k(z,x*) − k_zᵀ K⁻¹ k_* = Σ_{k ≤ N} k(z, x_k)·vext[k]: one kernel-evaluation pass, nothing stored
        HIPCHK(c->cdot.ensure(sizeof(double) * pad_up(c->M, 16)));
        const bool resident = c->resident(g);
        HIPCHK(g->events(EV_ACQ_END + 1));
        // The set's block-form q-EI state (blocks + chain) follows the model through real appends.  Entry i = number of rows appended
        // since the state's base.  If the appended point is the next FANTASY of the last batch (the picks appended for real, in
        // order), its column c_i(z) is in the chain already (it does not depend on the observed value): no pass over K_ZX.  Otherwise
        // the pass below runs and its column joins the chain as real entry i (the fantasies behind it are dropped).  The model's rows
        // since the base must be the chain's points, bit for bit; anything else resets the state.
        int chain_i = -1, chain_put = -1;
        abo_cand::Qei& Q = c->qei;
        std::vector<double> newx;
        if (Q.N >= 0 && (P != 1 || !resident || getenv("ABO_QEI_NO_CHAIN"))) Q = abo_cand::Qei();
        bool qok = false;
        { const int32_t r = qei_resync(g, c, c->synced_N, &qok); if (r) return r; }
        if (qok) {
            const int i = Q.nreal;
            std::vector<double> row(g->d);
            if ((int)g->ap_x.size() == g->d && Q.N + i == g->N - 1) {
                row = g->ap_x;                                     // the appended point as the host handed it over: no read-back, no wait
            } else {
                HIPCHK(hipMemcpyAsync(row.data(), g->st->Xraw.as<double>() + (Q.N + i) * g->d, sizeof(double) * g->d, hipMemcpyDeviceToHost, s));
                HIPCHK(wait_stream(s));
            }
            if (i < Q.nchain && !memcmp(row.data(), &Q.chain_x[(size_t)i * g->d], sizeof(double) * g->d)) chain_i = i;
            else if (i < Q.chain_rows) { chain_put = i; newx = row; }
            else Q = abo_cand::Qei();                                                                                  // no room: start over
        }
        g->tm.downdate_from_chain = chain_i >= 0 ? 1 : 0;
        HIPCHK(hipEventRecord(g->evs()[EV_ACQ_BEGIN], s));
        double pass_ms = 0.0;
        if (chain_i >= 0) {
            // the appended row's column keeps the resident K_ZX current for later passes
            HIPCHK(launch_cand_newcol(g->st->Xs.as<double>(), c->Z.as<double>(), c->Kzx.as<double>(), c->kzx_ld, c->M, (int)(g->N - 1),
                                      g->d, g->dp, g->prm.family, 1.0 / g->prm.ell, g->prm.sigma_f2, s));
            HIPCHK(hipEventRecord(g->evs()[EV_ACQ_SCORED], s));
            HIPCHK(launch_downdate(c->mu.as<double>(), c->var.as<double>(), c->qchain.as<double>() + (size_t)chain_i * Q.Mp, c->M,
                                   g->ap_beta, g->ap_s2, s));
            Q.chain_s[chain_i] = g->ap_s2;                         // what the stored variance was down-dated with
            Q.nreal = chain_i + 1;                                 // (the fantasies behind it stay: the next picks of the batch)
        }
        for (int q = 0; chain_i < 0 && q < P; ++q) {       // one rank-1 down-date per appended row, in append order
            const int64_t Rq = g->N - P + q;               // index of the appended row
            const double* vext = g->vext.as<double>() + (P > 1 ? (int64_t)q * g->st->cap : 0);
            const double s2 = P > 1 ? g->ap_s2v[q] : g->ap_s2, beta = P > 1 ? g->ap_betav[q] : g->ap_beta;
            if (resident) {
                // the appended row's column, then one streaming mat-vec over the resident K_ZX
                if (P == 1) {
                    HIPCHK(launch_cand_newcol(g->st->Xs.as<double>(), c->Z.as<double>(), c->Kzx.as<double>(), c->kzx_ld, c->M,
                                              (int)Rq, g->d, g->dp, g->prm.family, 1.0 / g->prm.ell, g->prm.sigma_f2, s));
                } else {
                    HIPCHK(launch_cand_newcol_grad(g->st->Xs.as<double>(), c->Z.as<double>(), c->Kzx.as<double>(), c->kzx_ld, c->M,
                                                   (int)Rq, (int)(g->npts - 1), q, g->d, g->dp, g->prm.family, 1.0 / g->prm.ell,
                                                   g->prm.sigma_f2, s));
                }
                HIPCHK(launch_cand_gemv(c->Kzx.as<double>(), c->kzx_ld, vext, (int)(Rq + 1), c->M, c->cdot.as<double>(), s));
            }
            if (!resident) { rc = column_from_kernel_values(g, c, vext, Rq, P, c->cdot.as<double>()); if (rc) return rc; }
            if (q == P - 1) HIPCHK(hipEventRecord(g->evs()[EV_ACQ_SCORED], s));
            HIPCHK(launch_downdate(c->mu.as<double>(), c->var.as<double>(), c->cdot.as<double>(), c->M, beta, s2, s));
            if (chain_put >= 0) {                                  // the pass's column joins the chain as real entry chain_put
                HIPCHK(hipMemcpyAsync(c->qchain.as<double>() + (size_t)chain_put * Q.Mp, c->cdot.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, s));
                Q.chain_x.resize((size_t)chain_put * g->d);
                Q.chain_x.insert(Q.chain_x.end(), newx.begin(), newx.end());
                Q.chain_s.resize(chain_put);
                Q.chain_s.push_back(s2);
                Q.nreal = Q.nchain = chain_put + 1;
            }
        }
        HIPCHK(wait_stream(s));
        pass_ms = ev_ms(g->evs()[EV_ACQ_BEGIN], g->evs()[EV_ACQ_SCORED]);
        g->tm.downdate_ms = pass_ms;
        g->tm.downdate_bytes = (resident && chain_i < 0) ? 8.0 * (double)g->N * (double)c->M * P : 0.0;
        c->dd_serial = P == 1 ? g->ap_serial : 0;
        c->dd_src = chain_i >= 0 ? 1 : 0;
        c->dd_chain = chain_i;
    }
    c->synced_N = g->N;
    return ABO_OK;
}

int32_t abo_cand_acq(abo_gp* g, abo_cand* c, int32_t kind, double p0, double best_y, int64_t idx_base, double* scores,
                     int32_t k, double* top_val, int64_t* top_idx, int32_t out_space) {
    return abo::cand_acq_ex(g, c, kind, p0, best_y, idx_base, scores, out_space, k, top_val, top_idx, out_space);
}

int32_t abo_cand_acq_mes(abo_gp* g, abo_cand* c, const double* ystar, int32_t S, int32_t ys_space, int64_t idx_base, double* scores,
                         int32_t k, double* top_val, int64_t* top_idx, int32_t out_space) {
    int32_t rc = mes_check_samples(ystar, S, ys_space, "abo_cand_acq_mes");
    if (rc) return rc;
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_acq_mes: null argument");
    if (k < 0) return fail(ABO_EINVAL, "abo_cand_acq_mes: k = %d is negative", k);
    if (k > 0 && (!top_val || !top_idx)) return fail(ABO_EINVAL, "abo_cand_acq_mes: k > 0 needs top_val and top_idx");
    rc = mes_check_handle(g, "abo_cand_acq_mes");
    if (rc) return rc;
    if (g->prm.device != c->device) return fail(ABO_EINVAL, "candidate set lives on device %d, model on %d", c->device, g->prm.device);
    HIPCHK(hipSetDevice(g->prm.device));
    AcqTerms t;
    rc = mes_terms(g, ystar, S, ys_space, &t);
    if (rc) return rc;
    return score_select(g, c, [&](double* sc_d, hipStream_t s) {
        return launch_score_mes(c->mu.as<double>(), c->var.as<double>(), c->M, t.ystar, S, sc_d, nullptr, nullptr, s);
    }, idx_base, scores, out_space, k, top_val, top_idx, out_space);
}

int32_t abo_cand_save(abo_gp* g, abo_cand* c) {
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_save: null argument");
    HIPCHK(hipSetDevice(g->prm.device));
    const size_t bytes = sizeof(double) * (c->M > 0 ? c->M : 1);
    HIPCHK(c->mu_bak.ensure(bytes));
    HIPCHK(c->var_bak.ensure(bytes));
    HIPCHK(hipMemcpyAsync(c->mu_bak.p, c->mu.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(c->var_bak.p, c->var.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(wait_stream(g->stream));
    c->bak_gen = c->synced_gen; c->bak_N = c->synced_N;
    return ABO_OK;
}

int32_t abo_cand_restore(abo_gp* g, abo_cand* c) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_restore: null argument");
    if (c->bak_N < 0) return fail(ABO_EINVAL, "abo_cand_restore: nothing saved");
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(hipMemcpyAsync(c->mu.p, c->mu_bak.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(c->var.p, c->var_bak.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(wait_stream(g->stream));
    c->synced_gen = c->bak_gen; c->synced_N = c->bak_N;
    return ABO_OK;
}

int32_t abo_cand_get(abo_gp* g, abo_cand* c, double* mu, double* var, int32_t out_space) {
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_get: null argument");
    HIPCHK(hipSetDevice(g->prm.device));
    if (mu) { int32_t rc = copy_out(mu, c->mu.p, sizeof(double) * c->M, out_space, g->stream); if (rc) return rc; }
    if (var) { int32_t rc = copy_out(var, c->var.p, sizeof(double) * c->M, out_space, g->stream); if (rc) return rc; }
    HIPCHK(wait_stream(g->stream));
    return ABO_OK;
}

int32_t abo_cand_point(abo_gp* g, abo_cand* c, int64_t idx, double* x, double* mu, double* var) {
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_point: null argument");
    if (idx < 0 || idx >= c->M) return fail(ABO_EINVAL, "abo_cand_point: index %lld outside 0..%lld", (long long)idx, (long long)c->M - 1);
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    PinStage pin(g->ctx);
    if (x) HIPCHK(pin.d2h(x, c->Z.as<double>() + idx * c->d, sizeof(double) * c->d, s));
    if (mu) HIPCHK(pin.d2h(mu, c->mu.as<double>() + idx, sizeof(double), s));
    if (var) HIPCHK(pin.d2h(var, c->var.as<double>() + idx, sizeof(double), s));
    HIPCHK(wait_stream(s));
    pin.flush();
    return ABO_OK;
}

int32_t abo_cand_exclude(abo_gp* g, abo_cand* c, int64_t idx) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_exclude: null argument");
    if (idx < 0 || idx >= c->M) return fail(ABO_EINVAL, "abo_cand_exclude: index %lld outside 0..%lld", (long long)idx, (long long)c->M - 1);
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const double excl[2] = {HUGE_VAL, 0.0};                 // μ = +Inf, σ² = 0: EI = PI = 0, UCB = −Inf
    HIPCHK(hipMemcpyAsync(c->mu.as<double>() + idx, &excl[0], sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->var.as<double>() + idx, &excl[1], sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

}  // extern "C"

const double* abo::cand_points(const abo_cand* c) { return c->Z.as<double>(); }
const double* abo::cand_mu(const abo_cand* c) { return c->mu.as<double>(); }
int64_t abo::cand_size(const abo_cand* c) { return c->M; }
int abo::cand_dim(const abo_cand* c) { return c->d; }
int abo::cand_device(const abo_cand* c) { return c->device; }
void abo::cand_sync(const abo_cand* c, CandSync* o) { *o = CandSync{c->synced_gen, c->synced_N, c->mu_epoch}; }
// c(z) = k(z, x*) − k(z, X)·u of the one-row append that made `g`, over the set (in sync with g): where the down-date left it when that
// can be said with certainty, else recomputed into tmp [pad_up(M, 16)] with the down-date's own kernels.  Queued on g's stream.
int32_t abo::cand_downdate_column(abo_gp* g, abo_cand* c, double* tmp, const double** col, int* route) {
    const abo_cand::Qei& Q = c->qei;
    if (c->dd_serial != 0 && c->dd_serial == g->ap_serial) {
        if (c->dd_src == 0 && c->cdot.p) { *col = c->cdot.as<double>(); *route = 0; return ABO_OK; }
        const int i = c->dd_chain;
        if (c->dd_src == 1 && i >= 0 && i < Q.nreal && Q.gen == g->st->gen && Q.N + i == g->N - 1 && c->qchain.p && (int)g->ap_x.size() == g->d &&
            (size_t)(i + 1) * g->d <= Q.chain_x.size() && !memcmp(g->ap_x.data(), &Q.chain_x[(size_t)i * g->d], sizeof(double) * g->d)) {
            *col = c->qchain.as<double>() + (size_t)i * Q.Mp; *route = 1;
            return ABO_OK;
        }
    }
    hipStream_t s = g->stream;
    const int64_t Rq = g->N - 1;
    const double* vext = g->vext.as<double>();
    if (c->resident(g)) {
        // (the set is in sync with g: column Rq of the resident K_ZX is the appended row's)
        HIPCHK(launch_cand_gemv(c->Kzx.as<double>(), c->kzx_ld, vext, (int)(Rq + 1), c->M, tmp, s));
    } else if (int32_t rc = column_from_kernel_values(g, c, vext, Rq, 1, tmp)) {
        return rc;
    }
    *col = tmp; *route = 2;
    return ABO_OK;
}
