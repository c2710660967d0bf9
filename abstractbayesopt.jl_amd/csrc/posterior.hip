// The chunked posterior pass of the single-device host driver and what feeds it: the choice of the contraction engine and of the chunk,
// the int8 engine's scratch and its residue planes of W, the pass itself (posterior) with the options the pruned selection's bound
// passes use, the all-output evaluation of a gradient-enhanced model (grad_eval_device) and the derivative posterior of a value-only
// one (deriv_eval_device), the timings they leave — and the entry points
// that are nothing but such a pass over the caller's points.  Host-side orchestration only; declared in abo_state.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "abo_state.h"
#include "abo_kernels.h"
#include "kgen_core.h"

using namespace abo;

namespace {

constexpr int OZ_AUTO_MIN_NP = 1280;  // below this the fp64 kernels win (tools/engine_crossover.py, profiles/r06_engine_crossover.txt: fp64/int8 = 0.97 at
                                      // 1024, 1.09 at 1280, 1.21 at 1536, 1.90 at 4096; round 2's engine crossed at 1536)

size_t oz_scratch_limit() {
    const char* e = getenv("ABO_OZ_SCRATCH_LIMIT_MB");
    return e ? (size_t)atoll(e) << 20 : ~(size_t)0;
}

// exponent of the row scaling of a gradient-enhanced model's derivative outputs: 2^t ≈ √(prior variance of a derivative output / σ_f²)
int oz_grad_exp(const abo_gp* g) {
    if (g->p_out <= 1) return 0;
    return (int)std::lrint(0.5 * std::log2(grad_prior_var(g) / g->prm.sigma_f2));
}

int64_t pick_chunk(const abo_gp* g, int64_t M, bool int8) {
    int64_t mc = g->prm.chunk;
    if (mc <= 0 && int8) {
        // int8 engine: 28 bytes of residue planes and residue products per (candidate, training point); measured at N = 8192:
        // 8192 candidates per chunk 597 ms, 16384 572, 32768 565, 65536 560 per C3 step — 65536 at N = 8192 (15 GB of scratch of the
        // 288), 32768 at N = 16384
        mc = ((int64_t)1 << 32) / (g->Np * (int64_t)sizeof(double));
        if (mc < 2048) mc = 2048;
        if (mc > 65536) mc = 65536;
    } else if (mc <= 0) {
        // ~1 GiB of K_XZ per chunk (measured at N = 8192, tools/chunk_sweep.sh: 2048 candidates per chunk 1072 ms,
        // 4096 1011, 8192 997, 16384 992-995, 32768 998, 65536 996 — small chunks pay launch tails in every kernel,
        // larger ones lose a little L2/MALL reuse of the candidate panels), at least 2048 and at most 65536 candidates
        mc = ((int64_t)1 << 30) / (g->Np * (int64_t)sizeof(double));
        if (mc < 2048) mc = 2048;
        if (mc > 65536) mc = 65536;
    }
    mc = pad_up(mc, TB);
    if (int8) {        // byte offsets inside one residue plane of a chunk stay below 2^31 (32-bit lane offsets in the generator and the DMA)
        const int64_t cap = (((int64_t)1 << 31) / pad_up(g->Np, 256)) / 256 * 256 - 256;
        if (mc > cap) mc = cap;
    }
    const int64_t mp = pad_up(M, TB);
    return mc < mp ? mc : mp;
}

// The int8 engine's scratch — 2 × n bytes per (candidate, factor row) of a chunk, and the n residue planes of W: when the device
// cannot give it (a shared or nearly full GPU), the chunk *Mc is halved down to 4096 candidates, and below that *oz comes back false:
// the call then runs on the fp64 kernels (8 bytes per pair of a chunk four times smaller) instead of failing.
int32_t oz_acquire(abo_gp* g, int nm, int64_t M, int64_t* Mc_io, bool* oz_io) {
    const int64_t Np = g->Np;
    int64_t Mc = *Mc_io;
    bool oz = *oz_io;
    if (oz) {
        if (g->oz_plan.n != nm) {                               // another moduli count: the cached planes of W belong to the old plan
            if (!oz_make_plan(nm, &g->oz_plan)) return fail(ABO_EINVAL, "contraction: %d moduli not supported", nm);
            g->oz_N = -1;
        }
        const int64_t q = pad_up(Np, 256);
        hipError_t e = g->oz_WR.ensure(oz_w_bytes(nm, (int)Np));
        if (e == hipSuccess) e = g->oz_sexp.ensure(sizeof(int) * q);
        if (e == hipSuccess) e = g->oz_badr.ensure(sizeof(int) * q);
        while (e == hipSuccess) {
            // ABO_OZ_SCRATCH_LIMIT_MB caps what the two chunk buffers may take together (a knob for shared devices; the tests use it
            // to walk this very path)
            const size_t kb = oz_k_bytes(nm, (int)Np, (int)Mc);
            e = 2 * kb > oz_scratch_limit() ? hipErrorOutOfMemory : g->oz_KR.ensure(kb);
            if (e == hipSuccess) e = g->oz_U.ensure(kb);
            if (e == hipSuccess) e = g->oz_badc.ensure(sizeof(int) * (pad_up(Mc, 256) + OZ_CTR_INTS));   // + the GEMM's tile counters
            if (e != hipErrorOutOfMemory || Mc <= 4096) break;
            (void)hipGetLastError();
            g->oz_KR.release(); g->oz_U.release();
            Mc = pad_up(Mc / 2, 256);
            e = hipSuccess;
        }
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            g->oz_KR.release(); g->oz_U.release(); g->oz_WR.release();
            g->oz_N = -1;
            oz = false;
            Mc = pick_chunk(g, M, false);
        } else HIPCHK(e);
    }
    *Mc_io = Mc;
    *oz_io = oz;
    return ABO_OK;
}

// residue planes of this view's W, once per model (cached on the handle until the storage generation or the view changes)
int32_t oz_planes_of_w(abo_gp* g) {
    hipStream_t s = g->stream;
    if (g->oz_gen != g->st->gen || g->oz_N != g->N) {
        PHASE_EVENT(g->evs()[EV_WPLANES_BEGIN], s);
        HIPCHK(oz_prepare_w(g->oz_plan, g->st->W.as<double>(), g->st->cap, (int)g->Np, (int)g->N, g->oz_WR.as<int8_t>(),
                            g->oz_sexp.as<int>(), g->oz_badr.as<int>(), s, g->p_out, oz_grad_exp(g)));
        PHASE_EVENT(g->evs()[EV_WPLANES_END], s);
        g->oz_gen = g->st->gen; g->oz_N = g->N;
        g->oz_prepare_pending = true;                               // both events recorded in THIS call: read with the posterior timings
    }
    return ABO_OK;
}

// the fields of OzVarArgs that the handle decides, on its own residue plan: the cached planes of W with their row scales and flags, the
// chunk scratch oz_acquire sized, the model's rows.  A call adds its chunk, its scale of K, its outputs — and, on a short plan, that
// plan's planes in their place.
OzVarArgs oz_handle_args(abo_gp* g) {
    OzVarArgs oa{};
    oa.plan = &g->oz_plan; oa.WR = g->oz_WR.as<int8_t>(); oa.sexp = g->oz_sexp.as<int>(); oa.bad_row = g->oz_badr.as<int>();
    oa.KR = g->oz_KR.as<int8_t>(); oa.U = g->oz_U.as<int8_t>(); oa.bad_col = g->oz_badc.as<int>(); oa.ctr_clean = &g->oz_ctr_clean;
    oa.Np = (int)g->Np; oa.nvalid = (int)g->N; oa.kper = g->p_out; oa.ktg = oz_grad_exp(g);
    return oa;
}

// moduli of the bound pass's residue plan: 8 (default), 9, 10 — a short plan with the guard of ozaki.hip — or 14: the handle's plan,
// exact contraction, as before the short plan existed.  ABO_PRUNE_BOUND_MODULI; any other value (11 – 13, below 8, text) is IGNORED and
// the default 8 used — the head generator is instantiated for these counts alone; the test hook refuses such a value with an error.
int prune_bound_moduli() {
    static const int env = [] {
        const char* e = getenv("ABO_PRUNE_BOUND_MODULI");
        const int v = e ? atoi(e) : 0;
        return (kgen_short_moduli(v) || v == 14) ? v : 8;
    }();
    if (g_prune_bound_moduli.load(std::memory_order_relaxed) > 0) return g_prune_bound_moduli.load(std::memory_order_relaxed);
    return env;
}

// A/B switch, read once: on, unless the variable begins with '0'.  The fp32 tail of a first bound level with the fused head reads its
// training points from the fp32 image one launch per pass writes (kgen_tail32.hip) instead of rounding the fp64 rows again in every
// workgroup.
bool tail32_stage() { static const bool on = [] { const char* e = getenv("ABO_TAIL32_STAGE"); return !(e && e[0] == '0'); }(); return on; }

}  // namespace

namespace abo {    // declared in abo_state.h

// the variable set to ANYTHING (an ignored value included), read once — or the hook
bool prune_bound_moduli_asked() {
    static const bool env = getenv("ABO_PRUNE_BOUND_MODULI") != nullptr;
    return env || g_prune_bound_moduli.load(std::memory_order_relaxed) != 0;
}

// k((z,q),(z,q)) of a gradient output: −2σ_f²φ'(0)/ℓ²  (φ'(0) = −1/2 SE, −5/6 Matérn-5/2, −7/10 Matérn-7/2)
double grad_prior_var(const abo_gp* g) {
    const double c = g->prm.family == ABO_KERNEL_SE ? 1.0 : (g->prm.family == ABO_KERNEL_MATERN52 ? 5.0 / 3.0 : 7.0 / 5.0);
    return c * g->prm.sigma_f2 / (g->prm.ell * g->prm.ell);
}

// which engine runs the contraction of a posterior call on this handle (int8 = true), and with how many moduli
bool wants_int8(const abo_gp* g, bool want_var, int pc, int* nmod) {
    if (!want_var || (pc != 1 && pc != g->p_out)) return false;
    int eng = g->oz_engine, nm = g->oz_nmod, de, dn;
    oz_defaults(&de, &dn);
    if (eng == ABO_CONTRACT_AUTO) eng = de;
    if (!nm) nm = dn;
    *nmod = nm;
    // int32 accumulation of the residue GEMMs is exact for k·2^14 < 2^31: beyond 65536 padded training points the engine is not
    // offered (the fp64 kernels take over, whatever was asked for)
    if (g->Np > 65536) return false;
    return eng == ABO_CONTRACT_INT8 || (eng == ABO_CONTRACT_AUTO && g->Np >= OZ_AUTO_MIN_NP);
}

int32_t posterior(abo_gp* g, const double* Zd, int64_t Mpts, int kind, double p0, double best_y, double* mu_out,
                  double* var_out, double* score_out, const PostOpts& o) {
    const int64_t M = Mpts * o.pc;                       // candidate rows
    hipStream_t s = g->stream;
    const int64_t Np = g->Np;
    const int T = (int)(Np / TB);
    const bool want_var = var_out || score_out;
    int nm = 0;
    bool oz = wants_int8(g, want_var, o.pc, &nm);
    int64_t Mc = pick_chunk(g, M, oz);
    { int32_t rc = oz_acquire(g, nm, M, &Mc, &oz); if (rc) return rc; }
    {
        const bool fused = oz && kgen_writes_residues(kgen_model_args(g, false), nm);
        if (o.rblocks > 0 && !(fused && !o.kstore && o.pc == 1)) return PRUNE_UNAVAILABLE;
        // the fp64 chunk of K_XZ is not materialised when the generator writes the residue planes itself
        if (!o.kstore && !fused) HIPCHK(g->Kxz.ensure(sizeof(double) * Mc * Np));
    }
    HIPCHK(g->partial.ensure(sizeof(double) * T * Mc));
    HIPCHK(g->mu_c.ensure(sizeof(double) * Mc));
    DevBuf& mut = o.level2 ? g->pr_mut2 : g->pr_mut;     // (the first level's μ̃ and ε of all candidates stay what abo_test_prune_mean reads)
    DevBuf& eps = o.level2 ? g->pr_eps2 : g->pr_eps;
    if (o.rblocks > 0) {
        HIPCHK(mut.ensure(sizeof(double) * M));
        HIPCHK(eps.ensure(sizeof(double) * M));
        HIPCHK(g->pr_nrm.ensure(sizeof(double) * 4));
    }
    const int64_t nchunk = (M + Mc - 1) / Mc;
    if (!o.more) {
        g->passes.clear();
        g->tm.var_gemm_launches = 0;
        g->oz_prepare_pending = false;
        g->tm.oz_prepare_ms = 0.0;                                  // planes cached from an earlier call: nothing spent in this one
    }
    const int64_t chunk0 = g->passes.empty() ? 0 : g->passes.back().chunk0 + g->passes.back().nchunk;
    HIPCHK(g->events(ev_chunk(chunk0 + nchunk, EVC_KGEN_BEGIN)));     // (one past the slots of the pass's last chunk)
    if (oz) { int32_t rc = oz_planes_of_w(g); if (rc) return rc; }
    // the bound pass on a short plan: its own planes of the first 256·rblocks rows of W, row scales and guards — rebuilt every call (one
    // row-scale and one quantiser launch over R × R; appends, abo_update, a changed R and shared factor storage would all have to
    // invalidate a cache)
    const bool head32 = o.head32 && o.tail32 && o.rblocks > 0 && oz && (int64_t)256 * o.rblocks <= g->npts && 256 * o.rblocks <= 2048;
    const int nb = o.rblocks > 0 && !head32 ? prune_bound_moduli() : 0;
    const bool shortp = nb > 0 && nb != g->oz_plan.n;
    const double sf2k = g->p_out > 1 ? (o.pc > 1 ? 2.0 : 1.5) * g->prm.sigma_f2 : g->prm.sigma_f2;
    if (shortp) {
        if (g->oz_plan_b.n != nb && !oz_make_plan(nb, &g->oz_plan_b)) return fail(ABO_EINVAL, "bound pass: %d moduli not supported", nb);
        const int rows = 256 * o.rblocks;
        const int64_t q = pad_up(Np, 256);
        HIPCHK(g->oz_WRb.ensure((size_t)nb * rows * q));
        HIPCHK(g->oz_sexpb.ensure(sizeof(int) * rows));
        HIPCHK(g->oz_badrb.ensure(sizeof(int) * rows));
        HIPCHK(g->oz_delta.ensure(sizeof(double) * rows));
        const int bK = oz_bound_kbits(g->oz_plan_b.eP, rows);
        g->pb_sK = oz_k_scale(sf2k, bK);
        g->pb_rows = rows;
        HIPCHK(oz_prepare_w_bound(g->oz_plan_b, g->oz_plan, g->st->W.as<double>(), g->st->cap, (int)Np, (int)g->N, rows, bK, g->pb_sK,
                                  oz_k_scale(sf2k), sf2k * (1.0 + 0x1p-40), g->oz_WRb.as<int8_t>(), g->oz_sexpb.as<int>(), g->oz_badrb.as<int>(),
                                  g->oz_delta.as<double>(), s));
    } else if (o.rblocks > 0) g->pb_rows = 0;
    if (o.rblocks > 0) g->ph_rows = head32 ? 256 * o.rblocks : 0;
    const OzPlan& plan = shortp ? g->oz_plan_b : g->oz_plan;
    g->passes.push_back({chunk0, nchunk, M, o.rblocks > 0 && (int64_t)256 * o.rblocks < g->N ? (int64_t)256 * o.rblocks : g->N, oz && !head32 ? plan.n : 0, head32});
    g->tm.contraction_engine = want_var ? (oz ? ABO_CONTRACT_INT8 : ABO_CONTRACT_FP64) : 0;
    g->tm.oz_nmod = oz ? g->oz_plan.n : 0;
    // (prune_plan: fewer row blocks than the model has, so the tail is never empty)
    if (o.rblocks > 0) HIPCHK(launch_tail_norms(g->st->Xs.as<double>(), g->alpha.as<double>(), (int)g->npts, g->dp, 256 * o.rblocks, g->pr_nrm.as<double>(), s));
    if (head32) {
        const int rows = 256 * o.rblocks;
        HIPCHK(g->pr_head.ensure(sizeof(double) * M));
        HIPCHK(g->pr_ssq.ensure(sizeof(double) * M));
        HIPCHK(g->pr_wf.ensure(sizeof(float) * rows * rows));
        HIPCHK(g->pr_hdl.ensure(sizeof(double) * 2 * rows));
        KgenHead32Args ha{};
        ha.Xs = g->st->Xs.as<double>(); ha.Z = Zd; ha.alpha = g->alpha.as<double>(); ha.W = g->st->W.as<double>(); ha.ldw = g->st->cap;
        ha.Wf = g->pr_wf.as<float>(); ha.delta = g->pr_hdl.as<double>(); ha.l1 = g->pr_hdl.as<double>() + rows;
        ha.head = g->pr_head.as<double>(); ha.ssq = g->pr_ssq.as<double>();
        ha.M = M; ha.N = (int)g->npts; ha.Np = (int)Np; ha.R = rows; ha.d = g->d; ha.dp = g->dp; ha.family = g->prm.family;
        ha.s = 1.0 / g->prm.ell; ha.sigma_f2 = g->prm.sigma_f2; ha.mean_c = g->prm.mean_c;
        // what δ covers of the FULL pass: its plan's exponent budget, the scale of its image of K, its reconstruction error
        ha.eP_full = g->oz_plan.eP; ha.sK_full = oz_k_scale(sf2k);
        ha.rec_full = (128.0 * g->oz_plan.n * g->oz_plan.n + 256.0 * g->oz_plan.n) * std::ldexp(1.0, g->oz_plan.eP - 91);
        // (one launch over all candidates, timed in the contraction slots of the pass's first chunk)
        PHASE_EVENT(g->evs()[ev_chunk(chunk0, EVC_CONTRACT_BEGIN)], s);
        HIPCHK(launch_kgen_head32(ha, s));
        PHASE_EVENT(g->evs()[ev_chunk(chunk0, EVC_CONTRACT_END)], s);
        g->tm.var_gemm_launches += 1;
    }
    // the tail's training points in fp32, once per pass (nothing cached across calls: the rule of the head's preparation launch); a
    // first level without the fused head keeps the in-kernel conversion, as every other pass keeps what it had
    const bool staged = head32 && tail32_stage();
    if (staged) {
        HIPCHK(g->pr_xf.ensure(sizeof(float) * tail32_stage_floats((int)g->npts, g->dp, 256 * o.rblocks)));
        HIPCHK(launch_tail32_stage(g->st->Xs.as<double>(), (int)g->npts, g->dp, 256 * o.rblocks, g->pr_xf.as<float>(), s));
    }
    for (int64_t c = 0; c < nchunk; ++c) {
        const int64_t j0 = c * Mc;
        const int64_t m = (M - j0) < Mc ? (M - j0) : Mc;
        const int mcp = (int)pad_up(m, TB);
        auto ev = [&](EvChunk slot) { return g->evs()[ev_chunk(chunk0 + c, slot)]; };
        double* kchunk = o.kstore ? o.kstore + j0 * o.ldstore : g->Kxz.as<double>();
        const int64_t ldk = o.kstore ? o.ldstore : Np;
        KgenArgs ka = kgen_model_args(g, true);
        ka.Z = Zd; ka.alpha = g->alpha.as<double>(); ka.Kout = kchunk;
        ka.mu = g->mu_c.as<double>(); ka.ldk = ldk; ka.M = Mpts; ka.j0 = j0; ka.Mc = mcp;
        ka.pc = o.pc; ka.point_major = o.point_major;
        // int8 engine: the generator writes the residue planes of the chunk itself (the fp64 K_XZ is then only materialised for a
        // caller that keeps it — the resident K_ZX of a candidate set)
        ka.res_kmax = 256 * o.rblocks;
        const bool fused = oz && kgen_writes_residues(ka, plan.n);
        if (fused) {
            const int64_t q = pad_up(Np, 256);
            ka.res = g->oz_KR.as<int8_t>(); ka.res_ld = q; ka.res_plane = pad_up(mcp, 256) * q;
            // (a gradient-enhanced model's scaled chunk is bounded by σ_f²·√2, its all-output chunk by 2σ_f²: the exponent the
            // contraction below is told, oa.sK)
            ka.res_bad = g->oz_badc.as<int>(); ka.res_n = plan.n;
            ka.res_sK = shortp ? g->pb_sK : oz_k_scale(sf2k);
            ka.res_ktg = oz_grad_exp(g);
            if (!o.kstore) ka.Kout = nullptr;
        } else ka.res_kmax = 0;
        PHASE_EVENT(ev(EVC_KGEN_BEGIN), s);
        if (!head32) HIPCHK(launch_kgen(ka, s));
        if (o.rblocks > 0) {
            KgenTailArgs kt{};
            kt.Xs = ka.Xs; kt.Z = Zd; kt.alpha = ka.alpha; kt.norms = g->pr_nrm.as<double>();
            kt.mu_tail = mut.as<double>(); kt.eps = eps.as<double>();
            kt.M = Mpts; kt.j0 = j0; kt.Mc = mcp; kt.N = (int)g->npts; kt.Np = (int)Np; kt.k0 = ka.res_kmax; kt.d = g->d; kt.dp = g->dp; kt.family = ka.family;
            kt.s = ka.s; kt.sigma_f2 = ka.sigma_f2; kt.mean_c = ka.mean_c;
            if (staged) kt.Xf = g->pr_xf.as<float>();
            HIPCHK(o.tail32 ? launch_kgen_tail32(kt, s) : launch_kgen_tail(kt, s));
        }
        PHASE_EVENT(ev(EVC_KGEN_END), s);
        if (head32) {
            // (head and sum of squares of every candidate are there already)
        } else if (oz) {
            OzVarArgs oa = oz_handle_args(g);
            oa.Kxz = kchunk; oa.ldk = ldk; oa.partial = g->partial.as<double>(); oa.ldp = Mc; oa.Mc = mcp;
            if (shortp) {           // the short plan's planes of W (row stride of the full planes), scales, flags and guards
                oa.plan = &g->oz_plan_b;
                oa.WR = g->oz_WRb.as<int8_t>(); oa.sexp = g->oz_sexpb.as<int>(); oa.bad_row = g->oz_badrb.as<int>();
                oa.delta = g->oz_delta.as<double>(); oa.w_plane = (int64_t)256 * o.rblocks * pad_up(Np, 256);
            }
            // a gradient-enhanced model's scaled chunk is bounded by σ_f²·√2 (oz_prepare_w), a StandardGP's by σ_f²
            // (derivative candidates against derivative training rows, both scaled: 2σ_f²)
            oa.sK = shortp ? g->pb_sK : oz_k_scale(sf2k);
            if (o.pc > 1) { oa.rmode = o.point_major ? 1 : 2; oa.rper = o.pc; oa.r0 = j0; oa.rpts = Mpts; }
            oa.ev_quant = phase_events() ? ev(EVC_OZ_QUANT_END) : nullptr; oa.ev_gemm = phase_events() ? ev(EVC_OZ_GEMM_END) : nullptr;
            oa.planes_ready = fused ? 1 : 0;
            oa.rblocks = o.rblocks;
            PHASE_EVENT(ev(EVC_CONTRACT_BEGIN), s);
            HIPCHK(launch_var_ozaki(oa, s));
            PHASE_EVENT(ev(EVC_CONTRACT_END), s);
            g->tm.var_gemm_launches += 1;
        } else if (want_var) {
            VarGemmArgs va{};
            va.W = g->st->W.as<double>(); va.Kxz = kchunk; va.partial = g->partial.as<double>();
            va.ldw = g->st->cap; va.ldk = ldk; va.ldp = Mc; va.Np = (int)Np; va.Mc = mcp; va.nvalid = (int)g->N;
            PHASE_EVENT(ev(EVC_CONTRACT_BEGIN), s);
            HIPCHK(launch_var_gemm(va, s));
            PHASE_EVENT(ev(EVC_CONTRACT_END), s);
            g->tm.var_gemm_launches += 1;
        }
        FinalizeArgs fa{};
        fa.partial = g->partial.as<double>(); fa.mu_in = g->mu_c.as<double>(); fa.mu_out = mu_out;
        fa.var_out = var_out; fa.score_out = score_out; fa.ldp = Mc; fa.j0 = j0; fa.M = M;
        fa.T = (var_out || score_out) && !head32 ? (o.rblocks > 0 && 2 * o.rblocks < T ? 2 * o.rblocks : T) : 0; fa.Mc = mcp; fa.kind = kind; fa.sigma_f2 = g->prm.sigma_f2;
        fa.p0 = p0; fa.best_y = best_y;
        fa.prior_grad = grad_prior_var(g); fa.pc = o.pc; fa.point_major = o.point_major; fa.Mpts = Mpts;
        if (o.rblocks > 0) { fa.mu_tail = mut.as<double>(); fa.mu_eps = eps.as<double>(); }
        if (head32) { fa.head_g = g->pr_head.as<double>(); fa.ssq_g = g->pr_ssq.as<double>(); }
        PHASE_EVENT(ev(EVC_EPILOGUE_BEGIN), s);
        HIPCHK(launch_finalize(fa, s));
        PHASE_EVENT(ev(EVC_EPILOGUE_END), s);
    }
    return ABO_OK;
}

// Gradient-enhanced model: per-point posterior mean of all P outputs (mu_d [M][P]), P×P covariance block (cov_d [M][P][P]) and
// GradientNormUCB score (sc_d [M]) of M points in DEVICE memory (any output may be null) — queued on the handle's stream, no
// synchronisation.  The arithmetic behind abo_predict_grad_cov (GradientGP.jl:936-971, gradNormUCB.jl:43-51) and behind the
// refinement rounds of a gradient-enhanced handle (refine.hip: launch_refine_lockstep_grad).
int32_t grad_eval_device(abo_gp* g, const double* Zd, int64_t M, double beta, double* mu_d, double* cov_d, double* sc_d) {
    hipStream_t s = g->stream;
    const int P = g->p_out;
    const int64_t Np = g->Np;
    // points per chunk: V chunk (rows·Np doubles) ≤ 256 MiB, rows padded to 128
    int64_t pts = (((int64_t)1 << 28) / (Np * (int64_t)sizeof(double))) / P;
    if (pts < 1) pts = 1;
    if (pts > M) pts = M;
    const int64_t rows_pad = pad_up(pts * P, TB);
    // V = L⁻¹K_XZ on the int8-residue engine when the handle's contraction says so (same rule as the variance calls): the residue
    // GEMMs and a reconstruction that writes V itself; a chunk whose scratch the device cannot give runs on the fp64 GEMM
    int nm = 0;
    bool oz = wants_int8(g, true, P, &nm);
    if (oz) {
        int64_t mc = rows_pad;
        int32_t rc = oz_acquire(g, nm, rows_pad, &mc, &oz);
        if (rc) return rc;
        if (oz && mc != rows_pad) oz = false;
    }
    HIPCHK(g->events(EV_BASE));
    g->oz_prepare_pending = false;
    if (oz) { int32_t rc = oz_planes_of_w(g); if (rc) return rc; }
    g->tm.contraction_engine = oz ? ABO_CONTRACT_INT8 : ABO_CONTRACT_FP64;
    g->tm.oz_nmod = oz ? g->oz_plan.n : 0;
    // int8 engine: the generator writes the residue planes of the chunk itself; the fp64 chunk is then not materialised
    const bool fused = oz && kgen_writes_residues(kgen_model_args(g, false), g->oz_plan.n);
    if (!fused) HIPCHK(g->Kxz.ensure(sizeof(double) * rows_pad * Np));
    HIPCHK(g->partial.ensure(sizeof(double) * rows_pad * Np));       // V
    HIPCHK(g->mu_c.ensure(sizeof(double) * rows_pad));
    for (int64_t p0 = 0; p0 < M; p0 += pts) {
        const int64_t np = (M - p0) < pts ? (M - p0) : pts;
        const int rows = (int)pad_up(np * P, TB);
        KgenArgs ka = kgen_model_args(g, true);
        ka.mean_c = 0.0;                                             // (every output's mean is its entry of mean_vec)
        ka.Z = Zd; ka.alpha = g->alpha.as<double>(); ka.Kout = g->Kxz.as<double>();
        ka.mu = g->mu_c.as<double>(); ka.ldk = Np; ka.M = M; ka.j0 = p0 * P; ka.Mc = rows;
        ka.pc = P; ka.point_major = 1;
        if (fused) {
            const int64_t q256 = pad_up(Np, 256);
            ka.Kout = nullptr;
            ka.res = g->oz_KR.as<int8_t>(); ka.res_ld = q256; ka.res_plane = pad_up(rows, 256) * q256;
            ka.res_bad = g->oz_badc.as<int>(); ka.res_n = g->oz_plan.n; ka.res_sK = oz_k_scale(2.0 * g->prm.sigma_f2);
            ka.res_ktg = oz_grad_exp(g);
        }
        HIPCHK(launch_kgen(ka, s));
        if (oz) {
            OzVarArgs oa = oz_handle_args(g);
            oa.Kxz = g->Kxz.as<double>(); oa.ldk = Np; oa.Mc = rows;
            oa.sK = oz_k_scale(2.0 * g->prm.sigma_f2);
            oa.planes_ready = fused ? 1 : 0;
            oa.rmode = 1; oa.rper = P; oa.r0 = p0 * P; oa.rpts = M;
            oa.Vout = g->partial.as<double>(); oa.ldv = Np;
            HIPCHK(launch_var_ozaki(oa, s));
        } else {
            GemmArgs a{};           // V[row][i] = Σ_k Kxz[row][k]·W[i][k]
            a.A = g->Kxz.as<double>(); a.lda = Np; a.B = g->st->W.as<double>(); a.ldb = g->st->cap;
            a.C = g->partial.as<double>(); a.ldc = Np; a.M = rows; a.N = (int)Np; a.K = (int)Np;
            a.kmode = K_B_LOWER; a.batch = 1; a.alpha = 1.0; a.beta = 0.0;       // W[i][k] = 0 for k > i: half the product
            HIPCHK(launch_gemm_nt(a, s));
        }
        GradCovArgs ca{};
        ca.V = g->partial.as<double>(); ca.mu_rows = g->mu_c.as<double>(); ca.ldv = Np; ca.R = (int)g->N; ca.p = P;
        ca.pt0 = p0; ca.prior0 = g->prm.sigma_f2; ca.prior_g = grad_prior_var(g); ca.beta = beta;
        ca.cov_out = cov_d; ca.mu_out = mu_d; ca.score_out = sc_d;
        HIPCHK(launch_grad_cov(ca, (int)np, s));
    }
    return ABO_OK;
}

// VALUE-ONLY model (p_out == 1): the same three outputs for the (f, ∇f) posterior of M points, p = d + 1 — mu_d [M][p], cov_d [M][p][p],
// sc_d [M] in DEVICE memory, any of them null; launches only.  The pt == 1 sibling of grad_eval_device: per chunk the cross-kernel
// generator of kgen_deriv.hip, V = K·L⁻ᵀ on the triangular fp64 MFMA product and the per-point epilogue of misc.hip.
// The contraction ALWAYS runs on the fp64 GEMM, whatever the handle's contraction says: the int8-residue engine scales the derivative
// query outputs of a gradient-enhanced factor by a per-row power of two that goes with that factor's own derivative rows
// (oz_grad_exp); the scaling for derivative outputs against a value-only factor is a piece of work of its own.
// Points per chunk: V ≤ 256 MiB as in grad_eval_device, capped by a positive abo_params.chunk.  Every row of V, every mean and every
// block is formed by the same instructions in the same order wherever the chunk boundaries fall (the small and the tiled GEMM kernel
// agree bit for bit: gemm.hip): the result does not depend on the chunk, or on the call.
// The chunks' phases are timed in the per-chunk event slots of a posterior pass (collect_posterior_timings reads them).
int32_t deriv_eval_device(abo_gp* g, const double* Zd, int64_t M, double beta, double* mu_d, double* cov_d, double* sc_d) {
    hipStream_t s = g->stream;
    const int P = g->d + 1;
    const int64_t Np = g->Np;
    int64_t pts = (((int64_t)1 << 28) / (Np * (int64_t)sizeof(double))) / P;
    if (g->prm.chunk > 0 && pts > g->prm.chunk) pts = g->prm.chunk;
    if (pts < 1) pts = 1;
    if (pts > M) pts = M;
    const int64_t rows_pad = pad_up(pts * P, TB);
    const int64_t nchunk = (M + pts - 1) / pts;
    g->passes.clear();
    g->tm.var_gemm_launches = 0;
    g->oz_prepare_pending = false;
    g->tm.oz_prepare_ms = 0.0;
    HIPCHK(g->events(ev_chunk(nchunk, EVC_KGEN_BEGIN)));
    g->passes.push_back({0, nchunk, M * P, g->N, 0, false});
    g->tm.contraction_engine = ABO_CONTRACT_FP64;
    g->tm.oz_nmod = 0;
    HIPCHK(g->Kxz.ensure(sizeof(double) * rows_pad * Np));
    HIPCHK(g->partial.ensure(sizeof(double) * rows_pad * Np));       // V
    HIPCHK(g->mu_c.ensure(sizeof(double) * rows_pad));
    for (int64_t c = 0; c < nchunk; ++c) {
        const int64_t p0 = c * pts;
        const int64_t np = (M - p0) < pts ? (M - p0) : pts;
        const int64_t rows = pad_up(np * P, TB);
        auto ev = [&](EvChunk slot) { return g->evs()[ev_chunk(c, slot)]; };
        KgenDerivArgs ka{};
        ka.Xs = g->st->Xs.as<double>(); ka.Z = Zd; ka.alpha = g->alpha.as<double>();
        ka.Kout = g->Kxz.as<double>(); ka.mu_rows = g->mu_c.as<double>(); ka.ldk = Np;
        ka.M = M; ka.pt0 = p0; ka.npts = (int)np; ka.rows_pad = rows;
        ka.N = (int)g->N; ka.Np = (int)Np; ka.d = g->d; ka.dp = g->dp; ka.family = g->prm.family;
        ka.s = 1.0 / g->prm.ell; ka.sigma_f2 = g->prm.sigma_f2; ka.mean_c = g->prm.mean_c;
        PHASE_EVENT(ev(EVC_KGEN_BEGIN), s);
        HIPCHK(launch_kgen_deriv(ka, s));
        PHASE_EVENT(ev(EVC_KGEN_END), s);
        GemmArgs a{};               // V[row][i] = Σ_k Kxz[row][k]·W[i][k]
        a.A = g->Kxz.as<double>(); a.lda = Np; a.B = g->st->W.as<double>(); a.ldb = g->st->cap;
        a.C = g->partial.as<double>(); a.ldc = Np; a.M = (int)rows; a.N = (int)Np; a.K = (int)Np;
        a.kmode = K_B_LOWER; a.batch = 1; a.alpha = 1.0; a.beta = 0.0;           // W[i][k] = 0 for k > i: half the product
        PHASE_EVENT(ev(EVC_CONTRACT_BEGIN), s);
        HIPCHK(launch_gemm_nt(a, s));
        PHASE_EVENT(ev(EVC_CONTRACT_END), s);
        g->tm.var_gemm_launches += 1;
        GradCovArgs ca{};
        ca.V = g->partial.as<double>(); ca.mu_rows = g->mu_c.as<double>(); ca.ldv = Np; ca.R = (int)g->N; ca.p = P;
        ca.pt0 = p0; ca.prior0 = g->prm.sigma_f2; ca.prior_g = grad_prior_var(g); ca.beta = beta;
        ca.cov_out = cov_d; ca.mu_out = mu_d; ca.score_out = sc_d;
        PHASE_EVENT(ev(EVC_EPILOGUE_BEGIN), s);
        HIPCHK(launch_grad_cov(ca, (int)np, s));
        PHASE_EVENT(ev(EVC_EPILOGUE_END), s);
    }
    return ABO_OK;
}

// phase times and algorithmic work of the call's posterior passes (what was launched: a bound pass counts its R rows, a survivor pass
// its survivors — with ONE exception: survivors whose scores were taken from the threshold pass, acq.hip: prune_survivors, are counted
// as if their pass had been launched; the pass of no chunks that stands for them adds work and no time)
void collect_posterior_timings(abo_gp* g, bool with_var) {
    double kx = 0, vg = 0, fi = 0, oq = 0, og = 0, oc = 0, work = 0, ozops = 0;
    const bool oz = with_var && g->tm.contraction_engine == ABO_CONTRACT_INT8;
    for (const abo_gp::PostPass& ps : g->passes) {
        for (int64_t c = 0; phase_events() && c < ps.nchunk; ++c) {
            auto ms = [&](EvChunk a, EvChunk b) { return ev_ms(g->evs()[ev_chunk(ps.chunk0 + c, a)], g->evs()[ev_chunk(ps.chunk0 + c, b)]); };
            kx += ms(EVC_KGEN_BEGIN, EVC_KGEN_END);
            // (a fused first-level head: one launch, timed in the first chunk's slot — the other chunks' slots hold older calls' events)
            if (with_var && (!ps.head32 || c == 0)) vg += ms(EVC_CONTRACT_BEGIN, EVC_CONTRACT_END);
            if (oz && !ps.head32) {
                oq += ms(EVC_CONTRACT_BEGIN, EVC_OZ_QUANT_END); og += ms(EVC_OZ_QUANT_END, EVC_OZ_GEMM_END); oc += ms(EVC_OZ_GEMM_END, EVC_CONTRACT_END);
            }
            fi += ms(EVC_EPILOGUE_BEGIN, EVC_EPILOGUE_END);
        }
        work += (double)ps.rows * (double)ps.rows * (double)ps.M;
        ozops += (double)ps.nmod * (double)ps.rows * (double)ps.rows * (double)ps.M;
    }
    g->tm.acq_kxz_ms = kx;
    g->tm.acq_var_gemm_ms = vg;
    g->tm.acq_finalize_ms = fi;
    g->tm.oz_quant_ms = oq; g->tm.oz_gemm_ms = og; g->tm.oz_crt_ms = oc;
    if (g->oz_prepare_pending) {
        g->tm.oz_prepare_ms = phase_events() ? ev_ms(g->evs()[EV_WPLANES_BEGIN], g->evs()[EV_WPLANES_END]) : 0.0;
        g->oz_prepare_pending = false;
    }
    // ALGORITHMIC int8 operations of the residue GEMMs: n moduli × the triangular product R²·M per pass (R(R+1)/2 multiply-adds per
    // candidate over the R rows of W the pass contracts — R = N but for a bound pass —, 2 operations each ≈ R²).  What the kernel issues
    // beyond that — the upper halves of its 256-wide diagonal blocks (of which it skips 6 of 16 units), padding of N and M to 256 — is
    // not credited.  The moduli are those each pass launched: a bound pass on its short plan counts that plan's.
    g->tm.oz_gemm_ops = oz ? ozops : 0.0;
    // algorithmic (triangular) flop of the contraction: R²·M per pass
    g->tm.var_gemm_flop = with_var ? work : 0.0;
}

}  // namespace abo

// ---- entry points that are a posterior pass over the caller's points ----------------------------------------------------------------------
extern "C" {

int32_t abo_predict(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, double* mu, double* var,
                    int32_t out_space) {
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (M < 0 || (M > 0 && !Z)) return fail(ABO_EINVAL, "abo_predict: bad candidate buffer");
    if (M == 0) return ABO_OK;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const double* Zd = nullptr;
    rc = stage_candidates(g, Z, M, z_space, &Zd);
    if (rc) return rc;
    double* mu_d = nullptr;
    double* var_d = nullptr;
    if (mu) {
        if (out_space == ABO_DEVICE) mu_d = mu;
        else { HIPCHK(g->mu_all.ensure(sizeof(double) * M)); mu_d = g->mu_all.as<double>(); }
    }
    if (var) {
        if (out_space == ABO_DEVICE) var_d = var;
        else { HIPCHK(g->var_all.ensure(sizeof(double) * M)); var_d = g->var_all.as<double>(); }
    }
    HIPCHK(hipEventRecord(g->evs()[EV_ACQ_BEGIN], s));
    rc = posterior(g, Zd, M, -1, 0.0, 0.0, mu_d, var_d, nullptr);
    if (rc) return rc;
    HIPCHK(hipEventRecord(g->evs()[EV_ACQ_SCORED], s));
    if (mu && out_space == ABO_HOST) { rc = copy_out(mu, mu_d, sizeof(double) * M, ABO_HOST, s); if (rc) return rc; }
    if (var && out_space == ABO_HOST) { rc = copy_out(var, var_d, sizeof(double) * M, ABO_HOST, s); if (rc) return rc; }
    HIPCHK(wait_stream(s));
    collect_posterior_timings(g, var != nullptr);
    g->tm.acq_topk_ms = 0.0;
    g->tm.acq_total_ms = ev_ms(g->evs()[EV_ACQ_BEGIN], g->evs()[EV_ACQ_SCORED]);
    return ABO_OK;
}

int32_t abo_predict_grad(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, double* mu, double* var,
                         int32_t out_space) {
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (g->p_out < 2) return fail(ABO_EINVAL, "abo_predict_grad: the model has no gradient outputs");
    if (M < 0 || (M > 0 && !Z)) return fail(ABO_EINVAL, "abo_predict_grad: bad candidate buffer");
    if (M == 0) return ABO_OK;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const int P = g->p_out;
    const double* Zd = nullptr;
    rc = stage_candidates(g, Z, M, z_space, &Zd);
    if (rc) return rc;
    double* mu_d = nullptr;
    double* var_d = nullptr;
    if (mu) { if (out_space == ABO_DEVICE) mu_d = mu; else { HIPCHK(g->mu_all.ensure(sizeof(double) * M * P)); mu_d = g->mu_all.as<double>(); } }
    if (var) { if (out_space == ABO_DEVICE) var_d = var; else { HIPCHK(g->var_all.ensure(sizeof(double) * M * P)); var_d = g->var_all.as<double>(); } }
    PostOpts all_outputs;
    all_outputs.pc = P;
    rc = posterior(g, Zd, M, -1, 0.0, 0.0, mu_d, var_d, nullptr, all_outputs);
    if (rc) return rc;
    if (mu && out_space == ABO_HOST) { rc = copy_out(mu, mu_d, sizeof(double) * M * P, ABO_HOST, s); if (rc) return rc; }
    if (var && out_space == ABO_HOST) { rc = copy_out(var, var_d, sizeof(double) * M * P, ABO_HOST, s); if (rc) return rc; }
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

int32_t abo_predict_grad_cov(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, double beta, double* mu,
                             double* cov, double* score, int32_t out_space) {
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    if (g->p_out < 2) return fail(ABO_EINVAL, "abo_predict_grad_cov: the model has no gradient outputs");
    if (M < 0 || (M > 0 && !Z)) return fail(ABO_EINVAL, "abo_predict_grad_cov: bad candidate buffer");
    if (M == 0) return ABO_OK;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const int P = g->p_out;
    const double* Zd = nullptr;
    rc = stage_candidates(g, Z, M, z_space, &Zd);
    if (rc) return rc;
    double* mu_d = nullptr; double* cov_d = nullptr; double* sc_d = nullptr;
    if (mu) { if (out_space == ABO_DEVICE) mu_d = mu; else { HIPCHK(g->mu_all.ensure(sizeof(double) * M * P)); mu_d = g->mu_all.as<double>(); } }
    if (cov) { if (out_space == ABO_DEVICE) cov_d = cov; else { HIPCHK(g->var_all.ensure(sizeof(double) * M * P * P)); cov_d = g->var_all.as<double>(); } }
    if (score) { if (out_space == ABO_DEVICE) sc_d = score; else { HIPCHK(g->score_all.ensure(sizeof(double) * M)); sc_d = g->score_all.as<double>(); } }
    rc = grad_eval_device(g, Zd, M, beta, mu_d, cov_d, sc_d);
    if (rc) return rc;
    if (mu && out_space == ABO_HOST) { rc = copy_out(mu, mu_d, sizeof(double) * M * P, ABO_HOST, s); if (rc) return rc; }
    if (cov && out_space == ABO_HOST) { rc = copy_out(cov, cov_d, sizeof(double) * M * P * P, ABO_HOST, s); if (rc) return rc; }
    if (score && out_space == ABO_HOST) { rc = copy_out(score, sc_d, sizeof(double) * M, ABO_HOST, s); if (rc) return rc; }
    HIPCHK(wait_stream(s));
    return ABO_OK;
}

int32_t abo_predict_deriv(abo_gp* g, const double* Z, int64_t M, int32_t d, int32_t z_space, double beta, double* mu,
                          double* cov, double* score, int32_t out_space) {
    // every refusal names the call and comes before any device work
    if (!g) return fail(ABO_EINVAL, "abo_predict_deriv: null handle");
    if (!g->fitted) return fail(ABO_EINVAL, "abo_predict_deriv: the surrogate is not conditioned on data yet (call abo_fit first)");
    if (g->p_out > 1) return fail(ABO_EINVAL, "abo_predict_deriv: the model is gradient-enhanced (abo_predict_grad_cov serves it)");
    if (d != g->d) return fail(ABO_EINVAL, "abo_predict_deriv: candidate dimension %d, model dimension %d", d, g->d);
    if (g->d > 32) return fail(ABO_EINVAL, "abo_predict_deriv: d = %d, at most 32 coordinates are supported", g->d);
    if (g->prm.family != ABO_KERNEL_SE && g->prm.family != ABO_KERNEL_MATERN52 && g->prm.family != ABO_KERNEL_MATERN72)
        return fail(ABO_EINVAL, "abo_predict_deriv: kernel family %d has no derivative posterior here (SE, Matern-5/2 and Matern-7/2 do)", g->prm.family);
    if (M < 0 || (M > 0 && !Z)) return fail(ABO_EINVAL, "abo_predict_deriv: bad candidate buffer (null Z or M < 0)");
    if (M == 0) return ABO_OK;
    int32_t rc = check_fitted(g, d);
    if (rc) return rc;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const int P = g->d + 1;
    const double* Zd = nullptr;
    rc = stage_candidates(g, Z, M, z_space, &Zd);
    if (rc) return rc;
    double* mu_d = nullptr; double* cov_d = nullptr; double* sc_d = nullptr;
    if (mu) { if (out_space == ABO_DEVICE) mu_d = mu; else { HIPCHK(g->mu_all.ensure(sizeof(double) * M * P)); mu_d = g->mu_all.as<double>(); } }
    if (cov) { if (out_space == ABO_DEVICE) cov_d = cov; else { HIPCHK(g->var_all.ensure(sizeof(double) * M * P * P)); cov_d = g->var_all.as<double>(); } }
    if (score) { if (out_space == ABO_DEVICE) sc_d = score; else { HIPCHK(g->score_all.ensure(sizeof(double) * M)); sc_d = g->score_all.as<double>(); } }
    HIPCHK(hipEventRecord(g->evs()[EV_ACQ_BEGIN], s));
    rc = deriv_eval_device(g, Zd, M, beta, mu_d, cov_d, sc_d);
    if (rc) return rc;
    HIPCHK(hipEventRecord(g->evs()[EV_ACQ_SCORED], s));
    if (mu && out_space == ABO_HOST) { rc = copy_out(mu, mu_d, sizeof(double) * M * P, ABO_HOST, s); if (rc) return rc; }
    if (cov && out_space == ABO_HOST) { rc = copy_out(cov, cov_d, sizeof(double) * M * P * P, ABO_HOST, s); if (rc) return rc; }
    if (score && out_space == ABO_HOST) { rc = copy_out(score, sc_d, sizeof(double) * M, ABO_HOST, s); if (rc) return rc; }
    HIPCHK(wait_stream(s));
    collect_posterior_timings(g, true);
    g->tm.acq_topk_ms = 0.0;
    g->tm.acq_total_ms = ev_ms(g->evs()[EV_ACQ_BEGIN], g->evs()[EV_ACQ_SCORED]);
    return ABO_OK;
}

}  // extern "C"
