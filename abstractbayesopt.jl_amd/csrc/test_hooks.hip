// The abo_test_* building blocks the GPU suite drives (include/abo_hip.h, last section) and nothing else: the one unit compiled with
// -DABO_TEST_HOOKS (the public header declares the hooks under it) and linked into libabo_hip_test.so only.  The overrides of the
// pruned selection (abo_state.h: g_prune_*) have their only writers here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "abo_oz_dev.h"
#include "abo_state.h"
#include "kgen_core.h"

using namespace abo;

extern "C" {

// value and gradient of the objective at M host points: one gradient-only refinement launch
static int32_t acq_grad_impl(abo_gp* g, const AcqTerms& t, const double* Z, int64_t M, int32_t d, double* f, double* grad);
int32_t abo_test_acq_grad_terms(abo_gp* g, const abo_acq_term* terms, int32_t nterms, const double* Z, int64_t M, int32_t d, double* f,
                                double* grad) {
    if (!g) return fail(ABO_EINVAL, "abo_test_acq_grad: null handle");
    int32_t rc = check_refinable(g, d, "abo_test_acq_grad");
    if (rc) return rc;
    AcqTerms t{};
    rc = make_terms(g, terms, nterms, &t, "abo_test_acq_grad");
    if (rc) return rc;
    if (M < 0 || M > 65535 || (M > 0 && (!Z || !f || !grad))) return fail(ABO_EINVAL, "abo_test_acq_grad: bad argument (M ≤ 65535)");
    if (M == 0) return ABO_OK;
    return acq_grad_impl(g, t, Z, M, d, f, grad);
}

static int32_t acq_grad_impl(abo_gp* g, const AcqTerms& t, const double* Z, int64_t M, int32_t d, double* f, double* grad) {
    int32_t rc;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const size_t ns = (size_t)M * d;
    HIPCHK(g->Zdev.ensure(sizeof(double) * (2 * ns + M)));
    double *sd = g->Zdev.as<double>(), *xd = sd + ns, *fd = xd + ns;
    HIPCHK(hipMemcpyAsync(sd, Z, sizeof(double) * ns, hipMemcpyHostToDevice, s));
    rc = refine_device(g, t, nullptr, sd, (int)M, refine_defaults(nullptr), xd, fd, nullptr, 1);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(grad, xd, sizeof(double) * ns, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(f, fd, sizeof(double) * M, hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

int32_t abo_test_acq_grad(abo_gp* g, int32_t kind, double p0, double best_y, const double* Z, int64_t M, int32_t d, double* f,
                          double* grad) {
    const abo_acq_term one{kind, 0, p0, best_y, 1.0};
    return abo_test_acq_grad_terms(g, &one, 1, Z, M, d, f, grad);
}

int32_t abo_test_mes_partials(int32_t device, const double* mu, const double* var, int64_t M, const double* ystar, int32_t S, double* f,
                              double* dmu, double* dvar) {
    if (M < 0 || (M > 0 && (!mu || !var || !f || !dmu || !dvar))) return fail(ABO_EINVAL, "abo_test_mes_partials: bad argument");
    int32_t rc = mes_check_samples(ystar, S, ABO_DEVICE, "abo_test_mes_partials");
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_score_mes(mu, var, M, ystar, S, f, dmu, dvar, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_acq_grad_mes(abo_gp* g, const double* ystar, int32_t S, const double* Z, int64_t M, int32_t d, double* f, double* grad) {
    int32_t rc = mes_check_samples(ystar, S, ABO_HOST, "abo_test_acq_grad_mes");
    if (rc) return rc;
    if (!g) return fail(ABO_EINVAL, "abo_test_acq_grad_mes: null handle");
    rc = check_refinable(g, d, "abo_test_acq_grad_mes");
    if (rc) return rc;
    rc = mes_check_handle(g, "abo_test_acq_grad_mes");
    if (rc) return rc;
    if (M < 0 || M > 65535 || (M > 0 && (!Z || !f || !grad))) return fail(ABO_EINVAL, "abo_test_acq_grad_mes: bad argument (M ≤ 65535)");
    if (M == 0) return ABO_OK;
    AcqTerms t;
    rc = mes_terms(g, ystar, S, ABO_HOST, &t);
    if (rc) return rc;
    return acq_grad_impl(g, t, Z, M, d, f, grad);
}

int32_t abo_test_acq_partials(int32_t device, const double* mu, const double* var, int64_t M, int32_t kind, double p0, double best_y,
                              double* f, double* dmu, double* dvar) {
    if (M < 0 || (M > 0 && (!mu || !var || !f || !dmu || !dvar))) return fail(ABO_EINVAL, "abo_test_acq_partials: bad argument");
    if (!plain_kind(kind)) return fail(ABO_EINVAL, "abo_test_acq_partials: unknown acquisition kind %d", kind);
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_score_partials(mu, var, f, dmu, dvar, M, kind, p0, best_y, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_prune_plan(int64_t rows, int64_t M, int32_t k, int32_t want_scores, int32_t kind, double p0, int32_t p_out, int32_t int8_fused,
                            int32_t d, int64_t* out) {
    if (!out) return fail(ABO_EINVAL, "abo_test_prune_plan: null argument");
    const PrunePlan pp = prune_plan(rows, M, k, want_scores != 0, kind, p0, p_out, int8_fused != 0, d);
    out[0] = pp.eligible; out[1] = pp.rblocks; out[2] = pp.k0; out[3] = pp.max_survivors;
    return ABO_OK;
}

int32_t abo_test_prune_force(int32_t rblocks, int32_t mode) {
    if (rblocks < 0 || mode < 0 || mode > 2) return fail(ABO_EINVAL, "abo_test_prune_force: rblocks = %d, mode = %d", rblocks, mode);
    g_prune_force_rblocks.store(rblocks);
    g_prune_force_mode.store(mode);
    return ABO_OK;
}

int32_t abo_test_prune_levels(int32_t pre_rblocks, int64_t level2_min) {
    if (pre_rblocks < -1 || level2_min < -1) return fail(ABO_EINVAL, "abo_test_prune_levels: pre_rblocks = %d, level2_min = %lld", pre_rblocks, (long long)level2_min);
    g_prune_pre_rblocks.store(pre_rblocks);
    g_prune_level2_min.store(level2_min);
    return ABO_OK;
}

int32_t abo_test_prune_tail32(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(ABO_EINVAL, "abo_test_prune_tail32: mode = %d (-1 = the environment's, 0 = fp64, 1 = fp32)", mode);
    g_prune_tail32.store(mode);
    return ABO_OK;
}

int32_t abo_test_prune_reuse(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(ABO_EINVAL, "abo_test_prune_reuse: mode = %d (-1 = the environment's, 0 = survivors evaluated again, 1 = taken from the threshold pass)", mode);
    g_prune_reuse.store(mode);
    return ABO_OK;
}

int32_t abo_test_prune_reused(abo_gp* g, int32_t* out) {
    if (!g || !out) return fail(ABO_EINVAL, "abo_test_prune_reused: null argument");
    *out = g->pr_reused ? 1 : 0;
    return ABO_OK;
}

int32_t abo_test_prune_head32(int32_t mode) {
    if (mode < -1 || mode > 1) return fail(ABO_EINVAL, "abo_test_prune_head32: mode = %d (-1 = the environment's, 0 = int8 head, 1 = fused fp32 head)", mode);
    g_prune_head32.store(mode);
    return ABO_OK;
}

int32_t abo_test_bound_head32(abo_gp* g, const double* Z, int64_t M, int32_t rblocks, double* head, double* ssq, double* delta, double* l1) {
    if (!g || !Z || !head || !ssq || !delta || !l1 || M <= 0 || rblocks <= 0) return fail(ABO_EINVAL, "abo_test_bound_head32: bad argument");
    { int32_t rc = check_fitted(g, g->d); if (rc) return rc; }
    if (g->p_out != 1) return fail(ABO_EINVAL, "abo_test_bound_head32: an ordinary model only");
    const int rows = 256 * rblocks;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    // every output with one sentinel behind M / behind row R: the kernels write nothing there
    ScratchBuf zd(g->prm.device, s), out(g->prm.device, s), wf(g->prm.device, s), dl(g->prm.device, s);
    HIPCHK(zd.b.ensure(sizeof(double) * M * g->d));
    HIPCHK(out.b.ensure(sizeof(double) * 2 * (M + 1)));
    HIPCHK(wf.b.ensure(sizeof(float) * rows * rows));
    HIPCHK(dl.b.ensure(sizeof(double) * 2 * (rows + 1)));
    const std::vector<double> fill(2 * (size_t)(M + 1), -7.0), fill_r(2 * (size_t)(rows + 1), -7.0);
    HIPCHK(hipMemcpyAsync(zd.b.p, Z, sizeof(double) * M * g->d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(out.b.p, fill.data(), sizeof(double) * fill.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dl.b.p, fill_r.data(), sizeof(double) * fill_r.size(), hipMemcpyHostToDevice, s));
    HIPCHK(wait_stream(s));
    OzPlan full;
    if (!oz_make_plan(OZ_DEFAULT_NMOD, &full)) return fail(ABO_EINVAL, "abo_test_bound_head32: no plan");
    KgenHead32Args ha{};
    ha.Xs = g->st->Xs.as<double>(); ha.Z = zd.b.as<double>(); ha.alpha = g->alpha.as<double>(); ha.W = g->st->W.as<double>(); ha.ldw = g->st->cap;
    ha.Wf = wf.b.as<float>(); ha.delta = dl.b.as<double>(); ha.l1 = dl.b.as<double>() + rows + 1;
    ha.head = out.b.as<double>(); ha.ssq = out.b.as<double>() + M + 1;
    ha.M = M; ha.N = (int)g->npts; ha.Np = (int)g->Np; ha.R = rows; ha.d = g->d; ha.dp = g->dp; ha.family = g->prm.family;
    ha.s = 1.0 / g->prm.ell; ha.sigma_f2 = g->prm.sigma_f2; ha.mean_c = g->prm.mean_c;
    ha.eP_full = full.eP; ha.sK_full = oz_k_scale(g->prm.sigma_f2);
    ha.rec_full = (128.0 * full.n * full.n + 256.0 * full.n) * std::ldexp(1.0, full.eP - 91);
    const hipError_t le = launch_kgen_head32(ha, s);
    if (le == hipErrorInvalidValue) return fail(ABO_EINVAL, "abo_test_bound_head32: %d rows on a model of %lld points", rows, (long long)g->npts);
    HIPCHK(le);
    // head / ssq: M + 1 doubles each, delta / l1: rows + 1 — the last of each is the sentinel (−7) as the kernels left it
    HIPCHK(hipMemcpyAsync(head, ha.head, sizeof(double) * (M + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ssq, ha.ssq, sizeof(double) * (M + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(delta, ha.delta, sizeof(double) * (rows + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(l1, ha.l1, sizeof(double) * (rows + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

int32_t abo_test_prune_plan_levels(int64_t rows, int64_t M, int32_t k, int32_t want_scores, int32_t kind, double p0, int32_t p_out,
                                   int32_t int8_fused, int32_t d, int64_t* out) {
    if (!out) return fail(ABO_EINVAL, "abo_test_prune_plan_levels: null argument");
    const PrunePlan pp = prune_plan(rows, M, k, want_scores != 0, kind, p0, p_out, int8_fused != 0, d);
    if (pp.rblocks0 >= pp.rblocks) return fail(ABO_EINVAL, "abo_test_prune_plan_levels: a first bound level of %d row blocks is not below the bound pass's %d", pp.rblocks0, pp.rblocks);
    out[0] = pp.eligible; out[1] = pp.rblocks; out[2] = pp.k0; out[3] = pp.max_survivors; out[4] = pp.rblocks0;
    return ABO_OK;
}

int32_t abo_test_prune_bound_moduli(int32_t n) {
    if (n != 0 && n != 14 && !kgen_short_moduli(n)) return fail(ABO_EINVAL, "abo_test_prune_bound_moduli: n = %d (0 = default, 8, 9, 10, 14)", n);
    g_prune_bound_moduli.store(n);
    return ABO_OK;
}

int32_t abo_test_prune_bound_plan(abo_gp* g, int32_t* sexp_b, double* delta, int64_t n_rows) {
    if (!g || !sexp_b || !delta || n_rows < 0) return fail(ABO_EINVAL, "abo_test_prune_bound_plan: bad argument");
    if (!g->pst.bound_rows || g->pb_rows <= 0 || n_rows > g->pb_rows)
        return fail(ABO_EINVAL, "abo_test_prune_bound_plan: the last abo_acq on this handle ran no bound pass on a short plan over %lld rows", (long long)n_rows);
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(hipMemcpyAsync(sexp_b, g->oz_sexpb.p, sizeof(int) * n_rows, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(delta, g->oz_delta.p, sizeof(double) * n_rows, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(wait_stream(g->stream));
    return ABO_OK;
}

int32_t abo_test_prune_bounds(abo_gp* g, double* out, int64_t M) {
    if (!g || !out || M < 0) return fail(ABO_EINVAL, "abo_test_prune_bounds: bad argument");
    if (!g->pst.bound_rows || g->pr_ub.cap < sizeof(double) * (size_t)M) return fail(ABO_EINVAL, "abo_test_prune_bounds: the last abo_acq on this handle ran no bound pass over %lld candidates", (long long)M);
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(hipMemcpyAsync(out, g->pr_ub.p, sizeof(double) * M, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(wait_stream(g->stream));
    return ABO_OK;
}

int32_t abo_test_prune_mean(abo_gp* g, double* mu, double* eps, int64_t M) {
    if (!g || !mu || !eps || M < 0) return fail(ABO_EINVAL, "abo_test_prune_mean: bad argument");
    if (!g->pst.bound_rows || g->pr_mut.cap < sizeof(double) * (size_t)M || g->pr_eps.cap < sizeof(double) * (size_t)M)
        return fail(ABO_EINVAL, "abo_test_prune_mean: the last abo_acq on this handle ran no bound pass over %lld candidates", (long long)M);
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(hipMemcpyAsync(mu, g->pr_mut.p, sizeof(double) * M, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(eps, g->pr_eps.p, sizeof(double) * M, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(wait_stream(g->stream));
    return ABO_OK;
}

int32_t abo_test_prune_head(abo_gp* g, double* head, double* ssq, int64_t M) {
    if (!g || !head || !ssq || M < 0) return fail(ABO_EINVAL, "abo_test_prune_head: bad argument");
    if (!g->pst.bound_rows || g->ph_rows <= 0 || g->pr_head.cap < sizeof(double) * (size_t)M || g->pr_ssq.cap < sizeof(double) * (size_t)M)
        return fail(ABO_EINVAL, "abo_test_prune_head: the last abo_acq on this handle ran no fused head over %lld candidates", (long long)M);
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(hipMemcpyAsync(head, g->pr_head.p, sizeof(double) * M, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(ssq, g->pr_ssq.p, sizeof(double) * M, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(wait_stream(g->stream));
    return ABO_OK;
}

int32_t abo_test_kappa_tail(int32_t device, int32_t family, const double* d2, double* out, int64_t n) {
    if (!d2 || !out || n < 0) return fail(ABO_EINVAL, "abo_test_kappa_tail: bad argument");
    if (family < ABO_KERNEL_SE || family > ABO_KERNEL_MATERN32) return fail(ABO_EINVAL, "abo_test_kappa_tail: unknown family");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_kappa_tail_test(family, d2, out, n, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_kappa_tail32(int32_t device, int32_t family, const double* d2, double* out, int64_t n) {
    if (!d2 || !out || n < 0) return fail(ABO_EINVAL, "abo_test_kappa_tail32: bad argument");
    if (family < ABO_KERNEL_SE || family > ABO_KERNEL_MATERN32) return fail(ABO_EINVAL, "abo_test_kappa_tail32: unknown family");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_kappa_tail32_test(family, d2, out, n, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_oz_plan(int32_t n, int32_t* p, double* tables, double* scal, int32_t* eP) {
    if (!p || !tables || !scal || !eP) return fail(ABO_EINVAL, "abo_test_oz_plan: null argument");
    OzPlan pl;
    if (!oz_make_plan(n, &pl)) return fail(ABO_EINVAL, "abo_test_oz_plan: %d moduli not supported (8 … %d)", n, OZ_MAXMOD);
    for (int l = 0; l < n; ++l) {
        p[l] = pl.p[l];
        tables[0 * OZ_MAXMOD + l] = pl.invp[l];
        tables[1 * OZ_MAXMOD + l] = pl.c26[l];
        tables[2 * OZ_MAXMOD + l] = pl.s1[l];
        tables[3 * OZ_MAXMOD + l] = pl.s2[l];
    }
    scal[0] = pl.P1; scal[1] = pl.P2; scal[2] = pl.invP;
    *eP = pl.eP;
    return ABO_OK;
}

int32_t abo_test_oz_contract(int32_t device, const double* W, int64_t ldw, int32_t Np, int32_t nvalid, const double* Kxz, int64_t ldk,
                             int32_t Mc, double kmax, int32_t nmod, double* partial, int64_t ldp) {
    if (!W || !Kxz || !partial) return fail(ABO_EINVAL, "abo_test_oz_contract: null argument");
    if (Np <= 0 || Np % TB || Mc <= 0 || Mc % TB || nvalid < 0 || nvalid > Np || ldw < Np || ldk < Np || ldp < Mc || !(kmax > 0.0))
        return fail(ABO_EINVAL, "abo_test_oz_contract: Np and Mc multiples of 128, nvalid <= Np, leading dimensions >= Np / Mc, kmax > 0");
    OzPlan pl;
    if (!oz_make_plan(nmod, &pl)) return fail(ABO_EINVAL, "abo_test_oz_contract: %d moduli not supported", nmod);
    HIPCHK(hipSetDevice(device));
    const int64_t q = pad_up(Np, 256), mq = pad_up(Mc, 256);
    ScratchBuf wr(device, nullptr), kr(device, nullptr), u(device, nullptr), ints(device, nullptr);
    HIPCHK(wr.b.ensure(oz_w_bytes(nmod, Np)));
    HIPCHK(kr.b.ensure(oz_k_bytes(nmod, Np, Mc)));
    HIPCHK(u.b.ensure(oz_k_bytes(nmod, Np, Mc)));
    HIPCHK(ints.b.ensure(sizeof(int) * (2 * q + mq + OZ_CTR_INTS)));
    int* sexp = ints.b.as<int>();
    HIPCHK(oz_prepare_w(pl, W, ldw, Np, nvalid, wr.b.as<int8_t>(), sexp, sexp + q, nullptr));
    OzVarArgs oa{};
    oa.plan = &pl; oa.Kxz = Kxz; oa.ldk = ldk; oa.WR = wr.b.as<int8_t>(); oa.sexp = sexp; oa.bad_row = sexp + q;
    oa.KR = kr.b.as<int8_t>(); oa.U = u.b.as<int8_t>(); oa.bad_col = sexp + 2 * q; oa.partial = partial; oa.ldp = ldp;
    oa.Np = Np; oa.Mc = Mc; oa.nvalid = nvalid; oa.sK = oz_k_scale(kmax);
    HIPCHK(launch_var_ozaki(oa, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_oz_contract_bound(int32_t device, const double* W, int64_t ldw, int32_t Np, int32_t nvalid, const double* Kxz, int64_t ldk,
                                   int32_t Mc, double kmax, int32_t nmod_b, int32_t rblocks, double* partial, int64_t ldp, double* delta) {
    if (!W || !Kxz || !partial || !delta) return fail(ABO_EINVAL, "abo_test_oz_contract_bound: null argument");
    const int rows = 256 * rblocks;
    if (Np <= 0 || Np % TB || Mc <= 0 || Mc % TB || nvalid < 0 || nvalid > Np || ldw < Np || ldk < Np || ldp < Mc || !(kmax > 0.0) ||
        rblocks <= 0 || rows > pad_up(Np, 256))
        return fail(ABO_EINVAL, "abo_test_oz_contract_bound: Np and Mc multiples of 128, nvalid <= Np, leading dimensions >= Np / Mc, kmax > 0, 256·rblocks <= pad256(Np)");
    OzPlan pl, full;
    if (!oz_make_plan(nmod_b, &pl) || !oz_make_plan(14, &full)) return fail(ABO_EINVAL, "abo_test_oz_contract_bound: %d moduli not supported", nmod_b);
    HIPCHK(hipSetDevice(device));
    const int64_t q = pad_up(Np, 256), mq = pad_up(Mc, 256);
    ScratchBuf wr(device, nullptr), kr(device, nullptr), u(device, nullptr), ints(device, nullptr);
    HIPCHK(wr.b.ensure((size_t)nmod_b * rows * q));
    HIPCHK(kr.b.ensure(oz_k_bytes(nmod_b, Np, Mc)));
    HIPCHK(u.b.ensure(oz_k_bytes(nmod_b, Np, Mc)));
    HIPCHK(ints.b.ensure(sizeof(int) * (2 * q + mq + OZ_CTR_INTS)));
    int* sexp = ints.b.as<int>();
    const int bK = oz_bound_kbits(pl.eP, rows);
    const int sKb = oz_k_scale(kmax, bK);
    HIPCHK(oz_prepare_w_bound(pl, full, W, ldw, Np, nvalid, rows, bK, sKb, oz_k_scale(kmax), kmax * (1.0 + 0x1p-40), wr.b.as<int8_t>(), sexp, sexp + q,
                              delta, nullptr));
    OzVarArgs oa{};
    oa.plan = &pl; oa.Kxz = Kxz; oa.ldk = ldk; oa.WR = wr.b.as<int8_t>(); oa.sexp = sexp; oa.bad_row = sexp + q;
    oa.KR = kr.b.as<int8_t>(); oa.U = u.b.as<int8_t>(); oa.bad_col = sexp + 2 * q; oa.partial = partial; oa.ldp = ldp;
    oa.Np = Np; oa.Mc = Mc; oa.nvalid = nvalid; oa.sK = sKb; oa.rblocks = rblocks; oa.delta = delta; oa.w_plane = (int64_t)rows * q;
    HIPCHK(launch_var_ozaki(oa, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// ---- the residue engine (csrc/ozaki.hip), stage by stage: every hook passes its arguments to ONE stage launcher on the null stream (the
// ---- GEMM hook with launches = 2: GEMM, reconstruction, GEMM — the counter protocol of production) and decides nothing itself
int32_t abo_test_oz_rowscale(int32_t device, const double* W, int64_t ldw, int32_t nrows, int32_t rows256, int32_t nmod, int32_t kper, int32_t ktg,
                             int32_t kbits, int32_t g_eP_full, int32_t g_sK_b, int32_t g_sK_full, double g_kmax, double g_rec_b, double g_rec_full,
                             int32_t* sexp, double* delta) {
    if (!W || !sexp) return fail(ABO_EINVAL, "abo_test_oz_rowscale: null argument");
    OzPlan pl;
    if (!oz_make_plan(nmod, &pl)) return fail(ABO_EINVAL, "abo_test_oz_rowscale: %d moduli not supported (8 … %d)", nmod, OZ_MAXMOD);
    if (rows256 <= 0 || rows256 % 256) return fail(ABO_EINVAL, "abo_test_oz_rowscale: rows256 must be a positive multiple of 256");
    if (delta && kper != 1) return fail(ABO_EINVAL, "abo_test_oz_rowscale: the guard is for kper = 1 (the bound pass is StandardGP only)");
    OzGuardArgs gd{};
    gd.delta = delta; gd.eP_full = g_eP_full; gd.sK_b = g_sK_b; gd.sK_full = g_sK_full; gd.kmax = g_kmax; gd.rec_b = g_rec_b; gd.rec_full = g_rec_full;
    HIPCHK(hipSetDevice(device));
    const hipError_t e = launch_oz_rowscale(W, ldw, nrows, rows256, pl.eP, sexp, kper, ktg, kbits, gd, nullptr);
    if (e == hipErrorInvalidValue)
        return fail(ABO_EINVAL, "abo_test_oz_rowscale: launch_oz_rowscale refused nrows = %d, rows256 = %d, ldw = %lld, kper = %d, ktg = %d, kbits = %d (0 <= nrows <= rows256, ldw >= nrows, kper >= 1, -60 <= ktg <= 900, 2 <= kbits <= 53)",
                    nrows, rows256, (long long)ldw, kper, ktg, kbits);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_oz_quant(int32_t device, const abo_test_oz_quant_args* t) {
    if (!t || !t->in || !t->out) return fail(ABO_EINVAL, "abo_test_oz_quant: null argument");
    OzQuantArgs q{};
    if (!oz_make_plan(t->nmod, &q.pl)) return fail(ABO_EINVAL, "abo_test_oz_quant: %d moduli not supported (8 … %d)", t->nmod, OZ_MAXMOD);
    // what the layout asks of the caller's buffer: whole 256-row blocks, planes that do not overlap
    if (t->rows_out <= 0 || t->rows_out % 256 || t->ld <= 0 || t->plane < (int64_t)t->rows_out * t->ld)
        return fail(ABO_EINVAL, "abo_test_oz_quant: rows_out a positive multiple of 256, plane >= rows_out * ld");
    q.in = t->in; q.ldin = t->ldin; q.rows_in = t->rows_in; q.cols_in = t->cols_in; q.rows_out = t->rows_out; q.cols_out = t->cols_out;
    q.lower = t->lower; q.srow = t->srow; q.sconst = t->sconst; q.kper = t->kper; q.ktg = t->ktg; q.rmode = t->rmode; q.rper = t->rper;
    q.rtg = t->rtg; q.r0 = t->r0; q.rpts = t->rpts; q.out = t->out; q.ld = t->ld; q.plane = t->plane; q.bad = t->bad;
    HIPCHK(hipSetDevice(device));
    const hipError_t e = launch_oz_quant(q, nullptr);
    if (e == hipErrorInvalidValue)
        return fail(ABO_EINVAL, "abo_test_oz_quant: launch_oz_quant refused rows %d of %d, cols %d of %d, ld = %lld, ldin = %lld, sconst = %d, ktg = %d, rtg = %d (cols_out a multiple of 16 and <= ld, ld of 64, rows_in <= rows_out, cols_in <= cols_out and ldin, scales inside the normal range)",
                    t->rows_in, t->rows_out, t->cols_in, t->cols_out, (long long)t->ld, (long long)t->ldin, t->sconst, t->ktg, t->rtg);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// PRECONDITION of the kernel, not checked here: the planes of WR are lower-triangular (byte [i][k] = 0 for k > i) — the GEMM skips
// the units of a diagonal block above the diagonal and stops each tile's k range at its diagonal block.  The bytes k >= 256·(row
// blocks covered) of a row are never read.
int32_t abo_test_oz_gemm(int32_t device, const int8_t* KR, const int8_t* WR, int32_t Np256, int32_t Mc256, int32_t nmod, int32_t rblocks,
                         int64_t w_plane, int8_t* U, int32_t launches) {
    if (!KR || !WR || !U) return fail(ABO_EINVAL, "abo_test_oz_gemm: null argument");
    OzPlan pl;
    if (!oz_make_plan(nmod, &pl)) return fail(ABO_EINVAL, "abo_test_oz_gemm: %d moduli not supported (8 … %d)", nmod, OZ_MAXMOD);
    if (launches != 1 && launches != 2) return fail(ABO_EINVAL, "abo_test_oz_gemm: launches = 1 or 2");
    if (Np256 <= 0 || Np256 % 256 || Mc256 <= 0 || Mc256 % 256 || rblocks < 0 || rblocks > Np256 / 256 ||
        (w_plane != 0 && w_plane < (int64_t)256 * oz_gemm_row_blocks(Np256, rblocks) * Np256))
        return fail(ABO_EINVAL, "abo_test_oz_gemm: Np256, Mc256 positive multiples of 256, 0 <= rblocks <= Np256 / 256, w_plane 0 or >= 256 * row blocks * Np256");
    HIPCHK(hipSetDevice(device));
    const int Ti = oz_gemm_row_blocks(Np256, rblocks);
    // the counters behind Mc256 flag ints, as launch_var_ozaki places them; zeroed ONCE
    ScratchBuf ints(device, nullptr), u1(device, nullptr), part(device, nullptr);
    HIPCHK(ints.b.ensure(sizeof(int) * ((size_t)Mc256 + OZ_CTR_INTS + Np256)));
    HIPCHK(hipMemsetAsync(ints.b.p, 0, sizeof(int) * ((size_t)Mc256 + OZ_CTR_INTS + Np256), nullptr));
    int* ctr = ints.b.as<int>() + Mc256;
    int8_t* first = U;
    if (launches == 2) {
        HIPCHK(u1.b.ensure((size_t)nmod * Ti * 256 * Mc256));
        first = u1.b.as<int8_t>();
    }
    hipError_t e = launch_oz_gemm(pl, KR, WR, first, Np256, Mc256, rblocks, w_plane, ctr, nullptr);
    if (e == hipErrorInvalidValue) return fail(ABO_EINVAL, "abo_test_oz_gemm: launch_oz_gemm refused Np256 = %d, Mc256 = %d, rblocks = %d", Np256, Mc256, rblocks);
    HIPCHK(e);
    if (launches == 2) {
        // a reconstruction of the first launch's U into a throw-away buffer resets the counters (ctr_reset), as it does between two
        // chunks of a posterior call; the second GEMM then runs WITHOUT a memset and writes the caller's U
        HIPCHK(part.b.ensure(sizeof(double) * (size_t)(2 * Ti) * Mc256));
        OzCrtLaunch c{};
        c.plan = &pl; c.U = first; c.Ti = Ti; c.sexp = ctr + OZ_CTR_INTS; c.sK = 0; c.Np = 256 * Ti; c.Mc = Mc256; c.nvalid = 256 * Ti;
        c.rper = 1; c.rpts = 1; c.ctr_reset = ctr; c.partial = part.b.as<double>(); c.ldp = Mc256;
        HIPCHK(launch_oz_crt(c, nullptr));
        HIPCHK(launch_oz_gemm(pl, KR, WR, U, Np256, Mc256, rblocks, w_plane, ctr, nullptr));
    }
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_oz_crt(int32_t device, const int8_t* U, int32_t Ti, int32_t nmod, const int32_t* sexp, int32_t sK, const int32_t* bad_row,
                        const int32_t* bad_col, int32_t Np, int32_t Mc, int32_t nvalid, int32_t rmode, int32_t rper, int32_t rtg, int64_t r0,
                        int64_t rpts, const double* delta, double* partial, int64_t ldp, double* V, int64_t ldv, int32_t generic,
                        int32_t* ctr_reset) {
    if (!U || !sexp || (!partial && !V)) return fail(ABO_EINVAL, "abo_test_oz_crt: null argument");
    OzPlan pl;
    if (!oz_make_plan(nmod, &pl)) return fail(ABO_EINVAL, "abo_test_oz_crt: %d moduli not supported (8 … %d)", nmod, OZ_MAXMOD);
    if (generic != 0 && generic != 1) return fail(ABO_EINVAL, "abo_test_oz_crt: generic = 0 or 1");
    OzCrtLaunch c{};
    c.plan = &pl; c.U = U; c.Ti = Ti; c.sexp = sexp; c.sK = sK; c.bad_row = bad_row; c.bad_col = bad_col; c.Np = Np; c.Mc = Mc; c.nvalid = nvalid;
    c.rmode = rmode; c.rper = rper; c.rtg = rtg; c.r0 = r0; c.rpts = rpts; c.ctr_reset = ctr_reset; c.delta = delta; c.partial = partial; c.ldp = ldp;
    c.V = V; c.ldv = ldv; c.generic = generic;
    HIPCHK(hipSetDevice(device));
    const hipError_t e = launch_oz_crt(c, nullptr);
    if (e == hipErrorInvalidValue)
        return fail(ABO_EINVAL, "abo_test_oz_crt: launch_oz_crt refused Ti = %d, Np = %d, Mc = %d, nvalid = %d, rmode = %d (Np, Mc positive multiples of 128, 0 <= nvalid <= Np, ldp >= Mc; V: ldv >= nvalid, nvalid <= 256 Ti, no delta; delta: rmode 0)",
                    Ti, Np, Mc, nvalid, rmode);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// oz_mod_pack4_mad on quads of integers: packed[i] = the four residue bytes of x[4i .. 4i+3] modulo p_l (l uniform: the asm takes −p
// from a scalar register, as the GEMM's epilogue does)
__global__ void __launch_bounds__(256) oz_modpack_test_kernel(const int* __restrict__ x, int64_t n4, double invp, int p, int* __restrict__ packed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int pu = __builtin_amdgcn_readfirstlane(p);
    packed[i] = oz_mod_pack4_mad(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3], invp, pu);
}

int32_t abo_test_oz_modpack(int32_t device, const int32_t* x, int64_t n4, int32_t l, int32_t* packed) {
    if (!x || !packed) return fail(ABO_EINVAL, "abo_test_oz_modpack: null argument");
    if (n4 < 0 || n4 > ((int64_t)1 << 28) || l < 0 || l >= OZ_MAXMOD) return fail(ABO_EINVAL, "abo_test_oz_modpack: 0 <= n4 <= 2^28, 0 <= l < %d", OZ_MAXMOD);
    if (n4 == 0) return ABO_OK;
    OzPlan pl;
    if (!oz_make_plan(OZ_MAXMOD, &pl)) return fail(ABO_EINVAL, "abo_test_oz_modpack: no plan");
    HIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(oz_modpack_test_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, nullptr, x, n4, pl.invp[l], pl.p[l], packed);
    HIPCHK(hipGetLastError());
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_oz_tickets(int32_t Ti, int32_t Tj, int32_t nmod, int32_t* tiles, int64_t* count) {
    if (!count) return fail(ABO_EINVAL, "abo_test_oz_tickets: null argument");
    const int64_t blocks = oz_gemm_tickets(Ti, Tj, nmod, tiles);
    if (blocks < 0) return fail(ABO_EINVAL, "abo_test_oz_tickets: launch_oz_gemm refuses Ti = %d, Tj = %d, nmod = %d (1 <= Ti <= 256, 1 <= Tj <= 2047, 1 <= nmod <= %d)", Ti, Tj, nmod, OZ_MAXMOD);
    *count = blocks;
    return ABO_OK;
}

int32_t abo_test_kappa(int32_t device, int32_t family, const double* d2, double* out, int64_t n) {
    if (!d2 || !out || n < 0) return fail(ABO_EINVAL, "abo_test_kappa: bad argument");
    if (family < ABO_KERNEL_SE || family > ABO_KERNEL_MATERN32) return fail(ABO_EINVAL, "abo_test_kappa: unknown family");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_kappa_test(family, d2, out, n, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_gemm_nt(int32_t device, const double* A, const double* B, double* C, int32_t M, int32_t N, int32_t K,
                         int64_t lda, int64_t ldb, int64_t ldc, double alpha, double beta) {
    if (!A || !B || !C) return fail(ABO_EINVAL, "abo_test_gemm_nt: null argument");
    if (M <= 0 || N <= 0 || K <= 0 || M % 128 || N % 128 || K % 16 || (lda & 1) || (ldb & 1))
        return fail(ABO_EINVAL, "abo_test_gemm_nt: M, N must be multiples of 128, K of 16, lda/ldb even");
    HIPCHK(hipSetDevice(device));
    GemmArgs a{};
    a.A = A; a.B = B; a.C = C; a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    a.kmode = K_FULL; a.batch = 1; a.alpha = alpha; a.beta = beta;
    HIPCHK(launch_gemm_nt(a, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// what the GEMM kernels assume of shapes and flags (no pointer is looked at): nullptr, or the text of the complaint
static const char* gemm_args_complaint(const GemmArgs& a) {
    if (a.M <= 0 || a.N <= 0 || a.M % TB || a.N % TB) return "M, N must be positive multiples of 128";
    if (a.K <= 0 || a.K % 16) return "K must be a positive multiple of 16";
    if (a.kmode < K_FULL || a.kmode > K_B_UPPER) return "unknown kmode";
    if (a.batch < 1 || a.ksplit < 0 || a.mrows < 0) return "batch >= 1, ksplit >= 0, mrows >= 0";
    if (a.ksplit && (a.K % 128 || a.ksplit % 128)) return "split-k: K and ksplit must be multiples of 128";
    if (a.ksplit && (a.batch != 1 || a.beta != 0.0 || a.Ct)) return "split-k: batch == 1, beta == 0, no Ct";
    return nullptr;
}

int32_t abo_test_gemm_path(int32_t M, int32_t N, int32_t K, int32_t kmode, int32_t lower_only, int32_t batch, int32_t ksplit,
                           int32_t mrows, int32_t in_place, int32_t* path) {
    if (!path) return fail(ABO_EINVAL, "abo_test_gemm_path: null argument");
    static double op[3];                       // three distinct addresses; never dereferenced
    GemmArgs a{};
    a.A = &op[0]; a.B = &op[1]; a.C = in_place ? &op[0] : &op[2];
    a.M = M; a.N = N; a.K = K; a.kmode = kmode; a.lower_only = lower_only; a.batch = batch; a.alpha = 1.0; a.ksplit = ksplit; a.mrows = mrows;
    if (const char* why = gemm_args_complaint(a)) return fail(ABO_EINVAL, "abo_test_gemm_path: %s", why);
    *path = gemm_nt_path(a);
    return ABO_OK;
}

int32_t abo_test_gemm_swz_map(int32_t T, int32_t G, int32_t Q, int32_t* ti, int32_t* tj) {
    if (!ti || !tj) return fail(ABO_EINVAL, "abo_test_gemm_swz_map: null argument");
    if (T < 1 || T > 4096 || G < 1 || Q < 0 || Q >= T * (T + 1) / 2) return fail(ABO_EINVAL, "abo_test_gemm_swz_map: 1 <= T <= 4096, G >= 1, 0 <= Q < T(T+1)/2");
    int i = -1, j = -1;
    gemm_swz_tile(T, G, Q, i, j);
    *ti = i; *tj = j;
    return ABO_OK;
}

int32_t abo_test_gemm_swz_q(int32_t tiles, int32_t L, int32_t* Q) {
    if (!Q) return fail(ABO_EINVAL, "abo_test_gemm_swz_q: null argument");
    if (tiles < 1 || L < 0 || L >= (tiles + 7) / 8 * 8) return fail(ABO_EINVAL, "abo_test_gemm_swz_q: tiles >= 1, 0 <= L < ceil(tiles / 8) * 8");
    *Q = gemm_swz_q(L, tiles);
    return ABO_OK;
}

int32_t abo_test_gemm_args(int32_t device, const double* A, const double* B, double* C, double* Ct, int64_t lda, int64_t ldb, int64_t ldc,
                           int64_t ldct, int64_t sA, int64_t sB, int64_t sC, int64_t sCt, int32_t M, int32_t N, int32_t K, int32_t kmode,
                           int32_t lower_only, int32_t batch, double alpha, double beta, int32_t ksplit, int32_t mrows, const int64_t* info,
                           int32_t* path) {
    if (!A || !B || !C || !path) return fail(ABO_EINVAL, "abo_test_gemm_args: null argument");
    GemmArgs a{};
    a.A = A; a.B = B; a.C = C; a.Ct = Ct; a.lda = lda; a.ldb = ldb; a.ldc = ldc; a.ldct = ldct; a.sA = sA; a.sB = sB; a.sC = sC; a.sCt = sCt;
    a.M = M; a.N = N; a.K = K; a.kmode = kmode; a.lower_only = lower_only; a.batch = batch; a.alpha = alpha; a.beta = beta; a.info = info;
    a.ksplit = ksplit; a.mrows = mrows;
    if (const char* why = gemm_args_complaint(a)) return fail(ABO_EINVAL, "abo_test_gemm_args: %s", why);
    if ((lda & 1) || (ldb & 1) || lda < K || ldb < K || ldc < N || (Ct && ldct < M) || ((sA | sB) & 1) || sA < 0 || sB < 0 || sC < 0 || sCt < 0)
        return fail(ABO_EINVAL, "abo_test_gemm_args: lda, ldb even and >= K, ldc >= N, ldct >= M, batch strides >= 0 (those of A and B even)");
    const int p = gemm_nt_path(a);
    if (p == GEMM_PATH_SKINNY && (kmode == K_A_LOWER || kmode == K_A_UPPER))
        return fail(ABO_EINVAL, "abo_test_gemm_args: the skinny split-k kernel knows K_FULL, K_B_LOWER and K_B_UPPER only");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_gemm_nt(a, nullptr));
    HIPCHK(wait_stream(nullptr));
    *path = p;
    return ABO_OK;
}

int32_t abo_test_qei_pass(int32_t device, const double* A, int64_t lda, int32_t rows16, const double* B, int64_t ldb, int64_t nB, int32_t K,
                          double alpha, double* C, int64_t ldc, int32_t kmode, int32_t ksplit, int64_t sC) {
    if (!A || !B || !C) return fail(ABO_EINVAL, "abo_test_qei_pass: null argument");
    if (lda < K || ldb < K || ldc < nB || sC < 0) return fail(ABO_EINVAL, "abo_test_qei_pass: lda, ldb >= K, ldc >= nB, sC >= 0");
    HIPCHK(hipSetDevice(device));
    const hipError_t e = launch_qei_pass(A, lda, rows16, B, ldb, nB, K, alpha, C, ldc, nullptr, kmode, ksplit, sC);
    if (e == hipErrorInvalidValue) return fail(ABO_EINVAL, "abo_test_qei_pass: launch_qei_pass refused rows16 = %d, nB = %lld, K = %d, lda = %lld, ldb = %lld, kmode = %d, ksplit = %d",
                                                rows16, (long long)nB, K, (long long)lda, (long long)ldb, kmode, ksplit);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_splitk_reduce(int32_t device, const double* P, int64_t ldp, int64_t sP, int32_t nz, int32_t rows, int32_t cols, int32_t K,
                               int32_t ksplit, int32_t kmode, double* out, int64_t ldo) {
    if (!P || !out) return fail(ABO_EINVAL, "abo_test_splitk_reduce: null argument");
    if (rows <= 0 || cols <= 0 || (cols & 1) || (ldp & 1) || (ldo & 1) || (sP & 1) || ldp < cols || ldo < cols || sP < 0 || nz < 1 || K <= 0 ||
        ksplit <= 0 || ksplit % 128 || (int64_t)nz * ksplit < K)
        return fail(ABO_EINVAL, "abo_test_splitk_reduce: rows > 0, cols > 0 and even, ldp / ldo / sP even, ldp, ldo >= cols, ksplit a multiple of 128, nz chunks covering K");
    if (kmode != K_FULL && kmode != K_B_LOWER && kmode != K_B_UPPER) return fail(ABO_EINVAL, "abo_test_splitk_reduce: kmode must be K_FULL, K_B_LOWER or K_B_UPPER");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_splitk_reduce(P, ldp, sP, nz, rows, cols, K, ksplit, kmode, out, ldo, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_var_gemm(int32_t device, const double* W, int64_t ldw, int32_t Np, int32_t nvalid, const double* Kxz, int64_t ldk, int32_t Mc,
                          double* partial, int64_t ldp, int32_t variant) {
    if (!W || !Kxz || !partial) return fail(ABO_EINVAL, "abo_test_var_gemm: null argument");
    if (Np <= 0 || Np % TB || Mc <= 0 || Mc % TB || nvalid < 0 || nvalid > Np || ldw < Np || ldk < Np || (ldw & 1) || (ldk & 1) || ldp < Mc)
        return fail(ABO_EINVAL, "abo_test_var_gemm: Np and Mc multiples of 128, nvalid <= Np, ldw / ldk even and >= Np, ldp >= Mc");
    if (variant != 0 && variant != 1) return fail(ABO_EINVAL, "abo_test_var_gemm: variant 0 (the launcher's rule) or 1 (the 128-row kernel)");
    HIPCHK(hipSetDevice(device));
    VarGemmArgs va{};
    va.W = W; va.Kxz = Kxz; va.partial = partial; va.ldw = ldw; va.ldk = ldk; va.ldp = ldp; va.Np = Np; va.Mc = Mc; va.nvalid = nvalid;
    HIPCHK(launch_var_gemm(va, nullptr, variant));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// launch_kgen with every field of KgenArgs as the caller gives it: no decision about shape, engine or dispatch is taken here
int32_t abo_test_kgen(int32_t device, const abo_test_kgen_args* t) {
    if (!t || !t->Xs || !t->Z) return fail(ABO_EINVAL, "abo_test_kgen: null argument");
    if (t->n_mean < 0 || t->n_mean > MAX_P || (t->n_mean > 0 && !t->mean_vec)) return fail(ABO_EINVAL, "abo_test_kgen: n_mean in [0, %d] with mean_vec given", MAX_P);
    KgenArgs a{};
    a.Xs = t->Xs; a.Z = t->Z; a.alpha = t->alpha; a.Kout = t->Kout; a.mu = t->mu; a.ldk = t->ldk; a.M = t->M; a.j0 = t->j0; a.Mc = t->Mc;
    a.N = t->N; a.Np = t->Np; a.d = t->d; a.dp = t->dp; a.family = t->family; a.s = t->s; a.sigma_f2 = t->sigma_f2;
    for (int q = 0; q < t->n_mean; ++q) a.mean_vec[q] = t->mean_vec[q];
    a.mean_c = t->n_mean > 0 ? t->mean_vec[0] : 0.0;
    a.pt = t->pt; a.pc = t->pc; a.point_major = t->point_major; a.dlogell = t->dlogell; a.rvalid = t->rvalid;
    a.res = t->res; a.res_ld = t->res_ld; a.res_plane = t->res_plane; a.res_bad = t->res_bad; a.res_n = t->res_n; a.res_sK = t->res_sK;
    a.res_ktg = t->res_ktg; a.res_kmax = t->res_kmax;
    HIPCHK(hipSetDevice(device));
    const hipError_t e = launch_kgen(a, nullptr);
    if (e == hipErrorInvalidValue)
        return fail(ABO_EINVAL, "abo_test_kgen: launch_kgen refused family = %d, dp = %d, pt = %d, dlogell = %d, res_n = %d, res_kmax = %d, Np = %d",
                    a.family, a.dp, a.pt, a.dlogell, a.res ? a.res_n : 0, a.res_kmax, a.Np);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// launch_kgen_deriv with the caller's arguments as they are
int32_t abo_test_kgen_deriv(int32_t device, const double* Xs, const double* alpha, const double* Z, double* Kout, double* mu_rows,
                            int64_t ldk, int64_t M, int64_t pt0, int32_t npts, int64_t rows_pad, int32_t N, int32_t Np, int32_t d, int32_t dp,
                            int32_t family, double s, double sigma_f2, double mean_c) {
    if (!Xs || !Z || !Kout) return fail(ABO_EINVAL, "abo_test_kgen_deriv: null argument");
    KgenDerivArgs a{};
    a.Xs = Xs; a.Z = Z; a.alpha = alpha; a.Kout = Kout; a.mu_rows = mu_rows; a.ldk = ldk; a.M = M; a.pt0 = pt0; a.npts = npts;
    a.rows_pad = rows_pad; a.N = N; a.Np = Np; a.d = d; a.dp = dp; a.family = family; a.s = s; a.sigma_f2 = sigma_f2; a.mean_c = mean_c;
    HIPCHK(hipSetDevice(device));
    const hipError_t e = launch_kgen_deriv(a, nullptr);
    if (e == hipErrorInvalidValue)
        return fail(ABO_EINVAL, "abo_test_kgen_deriv: launch_kgen_deriv refused family = %d, d = %d, dp = %d, N = %d, Np = %d, npts = %d, rows_pad = %lld",
                    family, d, dp, N, Np, npts, (long long)rows_pad);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_cand_newcol(int32_t device, const double* Xs, const double* Z, double* Kzx, int64_t ld, int64_t M, int32_t col, int32_t grad,
                             int32_t pt, int32_t q, int32_t d, int32_t dp, int32_t family, double s, double sigma_f2) {
    if (!Xs || !Z || !Kzx) return fail(ABO_EINVAL, "abo_test_cand_newcol: null argument");
    HIPCHK(hipSetDevice(device));
    const hipError_t e = grad ? launch_cand_newcol_grad(Xs, Z, Kzx, ld, M, col, pt, q, d, dp, family, s, sigma_f2, nullptr)
                              : launch_cand_newcol(Xs, Z, Kzx, ld, M, col, d, dp, family, s, sigma_f2, nullptr);
    if (e == hipErrorInvalidValue) return fail(ABO_EINVAL, "abo_test_cand_newcol: the launcher refused family = %d (grad = %d)", family, grad);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// ---- the factorisation family (csrc/chol.hip, and the blocked driver of api.hip), piece by piece: every hook passes its arguments to
// ---- ONE launcher (the panel pair: two) on the null stream and decides nothing about shape or dispatch
int32_t abo_test_chol_diag(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t r0, int64_t* info) {
    if (!K || !W || !WT || !info) return fail(ABO_EINVAL, "abo_test_chol_diag: null argument");
    if (r0 < 0 || ld < (int64_t)r0 + 128) return fail(ABO_EINVAL, "abo_test_chol_diag: r0 >= 0, ld >= r0 + 128");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_chol_diag(K, W, WT, ld, r0, info, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_chol_panel(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t r0, int32_t nrows, int32_t zero_rows,
                            int64_t* info) {
    if (!K || !W || !WT || !info) return fail(ABO_EINVAL, "abo_test_chol_panel: null argument");
    if (r0 < 0 || r0 % 128 || nrows < 0 || nrows % 16 || ld <= 0 || ld % 128 || ld < (int64_t)r0 + 128)
        return fail(ABO_EINVAL, "abo_test_chol_panel: r0 a multiple of 128, nrows of 16, ld of 128 and >= r0 + 128");
    HIPCHK(hipSetDevice(device));
    ScratchBuf ops(device, nullptr);
    HIPCHK(ops.b.ensure(TRSM_STREAM_BYTES));
    HIPCHK(launch_potf2_diag(K, W, WT, ld, r0, info, nullptr, ops.b.as<double>(), zero_rows != 0));
    if (nrows > 0) HIPCHK(launch_trsm_stream(K, ops.b.as<double>(), ld, r0, nrows, info, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_trtri_batched(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t nblocks, int64_t* info) {
    if (!K || !W || !WT || !info) return fail(ABO_EINVAL, "abo_test_trtri_batched: null argument");
    if (nblocks < 1 || ld < 128 * (int64_t)nblocks) return fail(ABO_EINVAL, "abo_test_trtri_batched: nblocks >= 1, ld >= 128 * nblocks");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_trtri_diag_batched(K, W, WT, ld, nblocks, info, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_chol_blocked(int32_t device, double* K, double* W, double* WT, int64_t ld, int32_t Np, int32_t sw, int32_t ss,
                              int32_t super_rows, int64_t* info) {
    if (!K || !W || !WT || !info) return fail(ABO_EINVAL, "abo_test_chol_blocked: null argument");
    if (Np <= 0 || Np % 128 || ld % 128 || ld < Np || sw <= 0 || sw % 128 || ss <= 0 || ss % 128 || ss % sw || super_rows < 0)
        return fail(ABO_EINVAL, "abo_test_chol_blocked: Np, ld, sw, ss positive multiples of 128, ld >= Np, ss a multiple of sw, super_rows >= 0");
    HIPCHK(hipSetDevice(device));
    ScratchBuf t(device, nullptr);
    const size_t tb = sizeof(double) * (size_t)Np * (size_t)Np;          // as abo_fit sizes the handle's T
    HIPCHK(t.b.ensure(tb > TRSM_STREAM_BYTES ? tb : TRSM_STREAM_BYTES));
    CholBlocking blk;
    blk.SW = sw; blk.SSmax = ss; blk.super_rows = super_rows;
    int32_t rc = chol_blocked(K, W, WT, t.b.as<double>(), ld, Np, info, blk, nullptr);
    if (rc) return rc;
    rc = trinv_blocked(K, W, WT, t.b.as<double>(), ld, Np, info, nullptr);
    if (rc) return rc;
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_trmv(int32_t device, const double* Wm, int64_t ld, const double* v, double* out, int32_t Np, int32_t lower) {
    if (!Wm || !v || !out) return fail(ABO_EINVAL, "abo_test_trmv: null argument");
    if (Np < 1 || (ld & 1) || ld < (int64_t)Np + (Np & 1) || (lower != 0 && lower != 1))
        return fail(ABO_EINVAL, "abo_test_trmv: Np >= 1, ld even and >= Np rounded up to even (the rows are read in pairs), lower 0 or 1");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_trmv(Wm, ld, v, out, Np, lower, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_tri_skinny(int32_t device, const double* Wm, int64_t ld, const double* V, double* out, int32_t N, int32_t k, int32_t lower) {
    if (!Wm || !V || !out) return fail(ABO_EINVAL, "abo_test_tri_skinny: null argument");
    if (N < 1 || k < 1 || k > APPEND_BATCH_MAX || (ld & 3) || ld < pad_up(N, 16) || (lower != 0 && lower != 1))
        return fail(ABO_EINVAL, "abo_test_tri_skinny: N >= 1, 1 <= k <= 64, ld a multiple of 4 and >= N rounded up to 16, lower 0 or 1");
    HIPCHK(hipSetDevice(device));
    const int kp = (int)pad_up(k, 16);
    ScratchBuf part(device, nullptr);
    HIPCHK(part.b.ensure(sizeof(double) * tri_skinny_part_doubles(N, kp)));
    HIPCHK(launch_tri_skinny(Wm, ld, V, out, part.b.as<double>(), N, kp, lower, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_live_views(abo_gp* gp, int64_t* out, int32_t cap, int32_t* n) {
    if (!gp || !out || !n || cap < 0) return fail(ABO_EINVAL, "abo_test_live_views: null argument");
    if (!gp->fitted || !gp->st) return fail(ABO_EINVAL, "abo_test_live_views: surrogate is not conditioned on data yet");
    std::lock_guard<std::mutex> lk(gp->st->mu);
    int32_t i = 0;
    for (const int64_t v : gp->st->live) {
        if (i < cap) out[i] = v;
        ++i;
    }
    *n = i;
    return ABO_OK;
}

int32_t abo_test_nlml_terms(int32_t device, const double* L, int64_t ld, const double* delta, const double* alpha, int32_t N, double* out) {
    if (!L || !delta || !alpha || !out) return fail(ABO_EINVAL, "abo_test_nlml_terms: null argument");
    if (N < 1 || ld < N) return fail(ABO_EINVAL, "abo_test_nlml_terms: N >= 1, ld >= N");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_nlml_terms(L, ld, delta, alpha, N, out, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_append(int32_t device, const abo_test_append_args* t) {
    if (!t || !t->L || !t->W || !t->WT || !t->krow || !t->lvec || !t->vvec || !t->alpha_old || !t->alpha_new || !t->vext || !t->delta ||
        !t->scal || !t->info)
        return fail(ABO_EINVAL, "abo_test_append: null argument");
    if (t->N < 0 || t->cap <= t->N || t->ld <= t->N) return fail(ABO_EINVAL, "abo_test_append: N >= 0, cap > N, ld > N");
    AppendArgs a{};
    a.L = t->L; a.W = t->W; a.WT = t->WT; a.ld = t->ld; a.krow = t->krow; a.lvec = t->lvec; a.vvec = t->vvec;
    a.alpha_old = t->alpha_old; a.alpha_new = t->alpha_new; a.vext = t->vext; a.delta = t->delta; a.N = t->N; a.cap = t->cap;
    a.kss = t->kss; a.scal = t->scal; a.info = t->info;
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_append(a, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// ---- the selection family (csrc/misc.hip): the same rule — every hook passes its arguments to ONE launcher on the null stream and
// ---- decides nothing about route or shape
int32_t abo_test_topk_plan(int64_t M, int32_t k, int64_t* out) {
    if (!out) return fail(ABO_EINVAL, "abo_test_topk_plan: null argument");
    const TopkPlan p = topk_plan(M, k);
    out[0] = p.path; out[1] = p.kreal; out[2] = p.slice; out[3] = p.pairs; out[4] = p.rounds; out[5] = p.passes;
    return ABO_OK;
}

int32_t abo_test_topk(int32_t device, const double* scores, int64_t M, int32_t k, int64_t idx_base, double* top_val, int64_t* top_idx,
                      int32_t* guards_ok) {
    if (!scores || !top_val || !top_idx || !guards_ok) return fail(ABO_EINVAL, "abo_test_topk: null argument");
    if (M < 0 || k < 0 || idx_base < 0) return fail(ABO_EINVAL, "abo_test_topk: M >= 0, k >= 0, idx_base >= 0");
    HIPCHK(hipSetDevice(device));
    // four buffers of exactly the entries the callers allocate, each followed by GUARD sentinel entries (every byte 0x5a; the
    // workspace itself starts as the same bytes: nothing of it may be read before it is written)
    constexpr int64_t GUARD = 1024;
    constexpr uint64_t SENTINEL = 0x5a5a5a5a5a5a5a5aull;
    const int64_t n = topk_workspace_entries(M, k), stride = n + GUARD;
    ScratchBuf ws(device, nullptr);
    HIPCHK(ws.b.ensure(sizeof(uint64_t) * 4 * stride));
    HIPCHK(hipMemsetAsync(ws.b.p, 0x5a, sizeof(uint64_t) * 4 * stride, nullptr));
    uint64_t* base = ws.b.as<uint64_t>();
    TopkWork w;
    w.keys[0] = base; w.keys[1] = base + stride;
    w.idx[0] = reinterpret_cast<int64_t*>(base + 2 * stride); w.idx[1] = reinterpret_cast<int64_t*>(base + 3 * stride);
    HIPCHK(launch_topk(scores, M, k, idx_base, w, top_val, top_idx, nullptr));
    std::vector<uint64_t> guards(4 * GUARD);
    for (int b = 0; b < 4; ++b)
        HIPCHK(hipMemcpyAsync(guards.data() + b * GUARD, base + b * stride + n, sizeof(uint64_t) * GUARD, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(wait_stream(nullptr));
    int32_t ok = 1;
    for (uint64_t g : guards) if (g != SENTINEL) ok = 0;
    *guards_ok = ok;
    return ABO_OK;
}

int32_t abo_test_prune_compact(int32_t device, const double* ub, int64_t M, const double* tau, double abs_margin, int64_t* sel, int64_t* count) {
    if (!ub || !tau || !sel || !count) return fail(ABO_EINVAL, "abo_test_prune_compact: null argument");
    HIPCHK(hipSetDevice(device));
    // one int of scan scratch per workgroup of the compaction; a count the launcher refuses gets one (it launches nothing)
    const bool fits = M > 0 && M < ((int64_t)1 << 31);
    ScratchBuf blk(device, nullptr);
    HIPCHK(blk.b.ensure(sizeof(int) * (size_t)(fits ? (M + PRUNE_SCAN_E - 1) / PRUNE_SCAN_E : 1)));
    const hipError_t e = launch_prune_compact(ub, M, tau, abs_margin, blk.b.as<int>(), sel, count, nullptr);
    if (e == hipErrorInvalidValue) return fail(ABO_EINVAL, "abo_test_prune_compact: launch_prune_compact refused M = %lld (1 <= M < 2^31)", (long long)M);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_prune_min_scatter(int32_t device, double* ub, const int64_t* sel, const double* ub2, int64_t n) {
    if (!ub || !sel || !ub2) return fail(ABO_EINVAL, "abo_test_prune_min_scatter: null argument");
    if (n < 0) return fail(ABO_EINVAL, "abo_test_prune_min_scatter: n >= 0");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_prune_min_scatter(ub, sel, ub2, n, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_prune_map(int32_t device, int64_t* top_idx, int32_t k, const int64_t* sel, int64_t idx_base) {
    if (!top_idx || !sel) return fail(ABO_EINVAL, "abo_test_prune_map: null argument");
    if (k < 0) return fail(ABO_EINVAL, "abo_test_prune_map: k >= 0");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_prune_map(top_idx, k, sel, idx_base, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_finalize(int32_t device, const abo_test_finalize_args* t) {
    if (!t) return fail(ABO_EINVAL, "abo_test_finalize: null argument");
    if ((t->T > 0 && !t->partial) || (!t->head_g && !t->mu_in) || (t->mu_tail && !t->mu_eps))
        return fail(ABO_EINVAL, "abo_test_finalize: null argument (partial with T > 0, mu_in without head_g, mu_eps with mu_tail)");
    if (t->T < 0 || t->Mc < 0 || t->j0 < 0 || t->M < 0 || t->ldp < t->Mc || t->pc < 1 || (t->pc > 1 && !t->point_major && t->Mpts <= 0))
        return fail(ABO_EINVAL, "abo_test_finalize: T, Mc, j0, M >= 0, ldp >= Mc, pc >= 1, Mpts > 0 for rows by outputs");
    FinalizeArgs a{};
    a.partial = t->partial; a.mu_in = t->mu_in; a.mu_out = t->mu_out; a.var_out = t->var_out; a.score_out = t->score_out;
    a.ldp = t->ldp; a.j0 = t->j0; a.M = t->M; a.T = t->T; a.Mc = t->Mc; a.kind = t->kind;
    a.sigma_f2 = t->sigma_f2; a.p0 = t->p0; a.best_y = t->best_y; a.prior_grad = t->prior_grad;
    a.pc = t->pc; a.point_major = t->point_major; a.Mpts = t->Mpts;
    a.mu_tail = t->mu_tail; a.mu_eps = t->mu_eps; a.head_g = t->head_g; a.ssq_g = t->ssq_g;
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_finalize(a, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_cand_gemv(int32_t device, const double* Kzx, int64_t ld, const double* v, int32_t n, int64_t M, double* c) {
    if (!Kzx || !v || !c) return fail(ABO_EINVAL, "abo_test_cand_gemv: null argument");
    if (n < 0 || M < 0 || (ld & 1) || ld < (int64_t)n + 1 || ((uintptr_t)Kzx & 15) || ((uintptr_t)v & 15))
        return fail(ABO_EINVAL, "abo_test_cand_gemv: n, M >= 0, ld even and >= n + 1, Kzx and v 16-byte aligned (the rows are read in pairs)");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_cand_gemv(Kzx, ld, v, n, M, c, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_downdate(int32_t device, double* mu, double* var, const double* c, int64_t M, double beta, double s2) {
    if (!mu || !var || !c) return fail(ABO_EINVAL, "abo_test_downdate: null argument");
    if (M < 0) return fail(ABO_EINVAL, "abo_test_downdate: M >= 0");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_downdate(mu, var, c, M, beta, s2, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_grad_cov(int32_t device, const double* V, const double* mu_rows, int64_t ldv, int32_t R, int32_t p, int64_t pt0,
                          double prior0, double prior_g, double beta, double* cov_out, double* mu_out, double* score_out, int32_t npoints) {
    if (!V || !mu_rows) return fail(ABO_EINVAL, "abo_test_grad_cov: null argument");
    if (p < 1 || R < 0 || ldv < R || pt0 < 0 || npoints < 0) return fail(ABO_EINVAL, "abo_test_grad_cov: p >= 1, R >= 0, ldv >= R, pt0 >= 0, npoints >= 0");
    GradCovArgs a{};
    a.V = V; a.mu_rows = mu_rows; a.ldv = ldv; a.R = R; a.p = p; a.pt0 = pt0; a.prior0 = prior0; a.prior_g = prior_g; a.beta = beta;
    a.cov_out = cov_out; a.mu_out = mu_out; a.score_out = score_out;
    HIPCHK(hipSetDevice(device));
    const hipError_t e = launch_grad_cov(a, npoints, nullptr);
    if (e == hipErrorInvalidValue) return fail(ABO_EINVAL, "abo_test_grad_cov: launch_grad_cov refused p = %d (C and m do not fit a workgroup's LDS)", p);
    HIPCHK(e);
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_gather_points(int32_t device, const double* Z, const int64_t* idx, int64_t idx_base, int32_t k, int32_t d, double* out) {
    if (!Z || !idx || !out) return fail(ABO_EINVAL, "abo_test_gather_points: null argument");
    if (k < 0 || d < 1) return fail(ABO_EINVAL, "abo_test_gather_points: k >= 0, d >= 1");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_gather_points(Z, idx, idx_base, k, d, out, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_pick_record(int32_t device, const double* tv, const int64_t* ti, int64_t idx_base, const double* Z, const double* mu,
                             int32_t d, double* rec) {
    if (!tv || !ti || !Z || !mu || !rec) return fail(ABO_EINVAL, "abo_test_pick_record: null argument");
    if (d < 1) return fail(ABO_EINVAL, "abo_test_pick_record: d >= 1");
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_pick_record(tv, ti, idx_base, Z, mu, d, rec, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

int32_t abo_test_score(int32_t device, const double* mu, const double* var, double* score, int64_t M, int32_t kind, double p0, double best_y) {
    if (!mu || !var || !score) return fail(ABO_EINVAL, "abo_test_score: null argument");
    if (M < 0 || !plain_kind(kind)) return fail(ABO_EINVAL, "abo_test_score: M >= 0 and a plain acquisition kind (got %d)", kind);
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_score(mu, var, score, M, kind, p0, best_y, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

// ---- the knowledge gradient's row kernel (csrc/kg.hip): the lines as handed in, one launcher, the null stream
int32_t abo_test_kg_lines(int32_t device, const double* a, const double* B, int64_t ldb, int32_t Ma, int32_t Mb, const double* self_a,
                          const double* self_b, double* val, int32_t* nenv) {
    if (!a || !B || !val || !nenv) return fail(ABO_EINVAL, "abo_test_kg_lines: null argument");
    if ((self_a == nullptr) != (self_b == nullptr)) return fail(ABO_EINVAL, "abo_test_kg_lines: self_a and self_b go together");
    if (Ma < 0 || Mb < 1 || Mb > KG_MAX_LINES || ldb < Mb)
        return fail(ABO_EINVAL, "abo_test_kg_lines: Ma >= 0, 1 <= Mb <= %d, ldb >= Mb", KG_MAX_LINES);
    KgArgs k{};
    k.a = a; k.B = B; k.ldb = ldb; k.den = nullptr; k.self_a = self_a; k.self_b = self_b; k.asign = 1.0; k.Ma = Ma; k.Mb = Mb;
    k.val = val; k.nenv = nenv;
    HIPCHK(hipSetDevice(device));
    HIPCHK(launch_kg_rows(k, nullptr));
    HIPCHK(wait_stream(nullptr));
    return ABO_OK;
}

}  // extern "C"
