// Greedy q-EI on a resident candidate set, host side (the kernels are qei.hip's): the set's block-form state (abo_cand::Qei, in
// abo_state.h) with its resync, continuation and chain rules, the per-shard steps abo::qei_* (abo_internal.h), the batch drivers — pick
// loop on the device, over shards, the plain loop — and the entry points abo_cand_qei* and abo_set_qei_block.  The set itself is
// cand.hip's.  Host-side orchestration only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>

#include "abo_state.h"

using namespace abo;

// Bring the set's block-form q-EI state (abo_cand::Qei) in line with a model of `rows_now` factor rows on the same storage: the rows
// appended since the state's base must be the chain's first points, bit for bit.  A model with FEWER appended rows than the chain
// has real entries (the caller rolled the set back — abo_cand_restore — and continues from an earlier point of the same lineage)
// keeps the chain: the entries beyond become fantasies again (a conditioning sequence in that order), and the blocks built on the
// longer model (their columns hold those conditionings) are dropped.  Anything else resets the state.  *ok: the state is usable.
int32_t abo::qei_resync(abo_gp* g, abo_cand* c, int64_t rows_now, bool* ok) {
    abo_cand::Qei& Q = c->qei;
    *ok = false;
    if (Q.N < 0) return ABO_OK;
    const int64_t i = rows_now - Q.N;
    if (Q.open || Q.gen != g->st->gen || i < 0 || i > Q.nreal) { Q = abo_cand::Qei(); return ABO_OK; }
    if (i > 0) {
        std::vector<double> rows((size_t)i * g->d);
        HIPCHK(hipMemcpyAsync(rows.data(), g->st->Xraw.as<double>() + Q.N * g->d, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, g->stream));
        HIPCHK(wait_stream(g->stream));
        if (memcmp(rows.data(), Q.chain_x.data(), sizeof(double) * rows.size())) { Q = abo_cand::Qei(); return ABO_OK; }
    }
    if (i < Q.nreal) {
        Q.nreal = (int)i;
        for (int b = 0; b < Q.nblk_cap; ++b)
            if (Q.blk_base[b] > Q.nreal)
                for (int t = 0; t < Q.T16; ++t) Q.slot_gidx[(size_t)b * Q.T16 + t] = -1;
    }
    *ok = true;
    return ABO_OK;
}

// ---- greedy q-EI, block form (qei.hip; include/abo_hip.h "block form"): per-shard steps + the driver ------------------------------
namespace {

// Julia's isless-descending order on scores (misc.hip: score_key): NaN first, then +Inf … −Inf with 0.0 before −0.0
uint64_t host_score_key(double v) {
    if (v != v) return ~0ull;
    uint64_t b;
    memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

std::atomic<int> g_qei_block{-1};
int qei_default_block() {
    int v = g_qei_block.load();
    if (v < 0) {
        const char* e = getenv("ABO_QEI_BLOCK");
        // 16 columns ride entirely under the K_ZX stream (6.3 TB/s), 32 cost 10 % more per pass — and halve how often a batch has to
        // build a block: over a 512-step cycle of config 5 with noisy observations one step in 8 rebuilt at T = 16, one in 16 at 32,
        // one in 27 at 64 (whose pass is MFMA-bound); mean step 1.13 / 0.98 / 0.99 ms (tools/c5_cycle.py, profiles/r06_c5_cycle.txt)
        v = e ? atoi(e) : 32;
        if (v < 0) v = 0;
        if (v > QEI_MAXT) v = QEI_MAXT;
        g_qei_block.store(v);
    }
    return v;
}

// chunk length of the split-k products against L⁻¹ (K⁻¹K_XT): about 16 chunks per column tile, so that the (tile, chunk) workgroups
// of the triangular range are a few times the device's CUs — the product streams L⁻¹ once and is HBM-bound
int qei_ksplit(int Np) {
    int ks = Np / 16 / 128 * 128;
    return ks < 128 ? 128 : ks;
}

struct QeiWork { double *P, *Ps, *KXT, *V, *U, *Ct; int ks, nz; size_t bytes; };
QeiWork qei_carve(void* base, int T16, int d, int dp, int Np) {
    QeiWork w{};
    w.ks = qei_ksplit(Np);
    w.nz = (Np + w.ks - 1) / w.ks;
    char* p = static_cast<char*>(base);
    auto take = [&](size_t n) { double* r = reinterpret_cast<double*>(p); p += (n * sizeof(double) + 255) / 256 * 256; return r; };
    w.P = take((size_t)T16 * d);
    w.Ps = take((size_t)T16 * dp);
    w.KXT = take((size_t)T16 * Np);
    w.V = take((size_t)T16 * Np);
    w.U = take((size_t)T16 * Np);
    w.Ct = take((size_t)w.nz * T16 * Np);
    w.bytes = (size_t)(p - static_cast<char*>(base));
    return w;
}

// The block slots are keyed by GLOBAL candidate index = idx_base + local index.  A caller that passes another idx_base than the one
// the slots were keyed with (a continuation from an earlier batch, or a change inside a batch) would match a pick against another
// candidate's covariance column: the slots are dropped (the chain is per local candidate and stays); the next pick builds a block.
int32_t qei_rebase(abo_cand* c, int64_t idx_base) {
    abo_cand::Qei& Q = c->qei;
    if (idx_base < 0) return fail(ABO_EINVAL, "q-EI: idx_base = %lld", (long long)idx_base);
    if (Q.idx_base != idx_base) {
        if (Q.idx_base >= 0) Q.slot_gidx.assign(Q.slot_gidx.size(), -1);
        Q.idx_base = idx_base;
    }
    return ABO_OK;
}

int qei_find_slot(const abo_cand* c, int64_t gidx) {
    const std::vector<int64_t>& v = c->qei.slot_gidx;
    for (size_t i = 0; i < v.size(); ++i) if (v[i] == gidx) return (int)i;
    return -1;
}

// The open rule of a set's block state (qei_begin, qei_mc_open): it continues when its base plus (some of) its real entries IS this
// model (rows compared bit for bit: qei_resync), with the same Mp and room for q more chain entries; else it starts afresh.  Another
// block size starts it afresh too (rekey = false) or only re-keys the ring of blocks, keeping the chain (rekey = true).
int32_t qei_open_state(abo_gp* g, abo_cand* c, int T16, int64_t Mp, int q, bool rekey) {
    abo_cand::Qei& Q = c->qei;
    bool cont = false;
    if (Q.N >= 0 && ((!rekey && Q.T16 != T16) || Q.Mp != Mp || getenv("ABO_QEI_NO_REUSE"))) Q = abo_cand::Qei();
    { const int32_t r = qei_resync(g, c, g->N, &cont); if (r) return r; }
    if (cont && Q.nreal + q > QEI_MAXQ) cont = false;
    if (!cont) {
        Q = abo_cand::Qei();
        Q.gen = g->st->gen; Q.N = g->N; Q.Mp = Mp;
        Q.nblk_cap = 4;                                    // ring of blocks: a pick outside all of them rebuilds the oldest
    }
    if (!cont || Q.T16 != T16) {
        Q.T16 = T16; Q.next_blk = 0;
        Q.slot_gidx.assign((size_t)Q.nblk_cap * T16, -1);
        Q.slot_x.assign((size_t)Q.nblk_cap * T16 * c->d, 0.0);
        Q.blk_base.assign(Q.nblk_cap, 0);
    }
    return ABO_OK;
}

// The first failure of a batch keeps its text across the roll-back: note() takes it from the thread's error slot before the calls
// that undo the batch (qei_end, the restoring copies) may write that slot again, report() puts it back with its code.
struct FirstError {
    std::string text;
    void note(int32_t rc) { if (rc && text.empty()) text = last_error_text(); }
    int32_t report(int32_t rc) const { return fail(rc, "%s", text.c_str()); }
};

// The one shard of a batch on a single handle: the set's own record block, read back on the handle's stream.
struct OneShard {
    abo_gp* gp[1]; abo_cand* cd[1]; int64_t lo[1];
    QeiShards S;
    OneShard(abo_gp* g, abo_cand* c, int64_t idx_base) : gp{g}, cd{c}, lo{idx_base} {
        S.n = 1; S.gp = gp; S.cd = cd; S.lo = lo;
        S.run = [](const std::function<int32_t(int)>& f) { return f(0); };
        S.rec = [c](int) { return c->qrec.as<double>(); };
        S.gather = [g, c](size_t words, double* out) -> int32_t {
            HIPCHK(hipMemcpyAsync(out, c->qrec.p, sizeof(double) * words, hipMemcpyDeviceToHost, g->stream));
            HIPCHK(wait_stream(g->stream));
            return ABO_OK;
        };
    }
    OneShard(const OneShard&) = delete;                    // (S points into this object)
};

}  // namespace

int32_t abo::qei_eligible(abo_gp* g, abo_cand* c, int q) {
    if (!g || !c) return fail(ABO_EINVAL, "q-EI: null argument");
    int32_t rc = check_fitted(g, c->d);
    if (rc) return rc;
    if (g->prm.device != c->device) return fail(ABO_EINVAL, "candidate set lives on device %d, model on %d", c->device, g->prm.device);
    if (!c->in_sync(g)) return fail(ABO_EINVAL, "q-EI: the candidate set is not in sync with this model (abo_cand_refresh / abo_cand_downdate)");
    if (g->p_out > 1) return fail(ABO_EINVAL, "q-EI, block form: gradient-enhanced models take the plain loop");
    if (c->M > 0 && !c->resident(g)) return fail(ABO_EINVAL, "q-EI, block form: K_ZX of the set is not resident");
    if (q < 1 || q > QEI_MAXQ) return fail(ABO_EINVAL, "q-EI, block form: q = %d outside 1..%d", q, QEI_MAXQ);
    if ((size_t)QEI_MAXT * c->d * sizeof(double) > 65536) return fail(ABO_EINVAL, "q-EI, block form: d = %d > 128 takes the plain loop", c->d);
    return ABO_OK;
}

int32_t abo::qei_begin(abo_gp* g, abo_cand* c, int q, int T, bool snapshot) {
    int32_t rc = abo::qei_eligible(g, c, q);
    if (rc) return rc;
    if (T <= 0) T = qei_default_block();
    if (T < 1) return fail(ABO_EINVAL, "q-EI, block form: block size 0 (the plain loop is a different call)");
    if (T > QEI_MAXT) T = QEI_MAXT;
    HIPCHK(hipSetDevice(g->prm.device));
    abo_cand::Qei& Q = c->qei;
    const int T16 = (int)pad_up(T, 16);
    const int64_t Mp = pad_up(c->M > 0 ? c->M : 1, TB);
    hipStream_t s = g->stream;
    { const int32_t r = qei_open_state(g, c, T16, Mp, q, /*rekey=*/false); if (r) return r; }
    HIPCHK(c->qblk.ensure(sizeof(double) * (size_t)Q.nblk_cap * T16 * Mp));
    // chain rows: the real entries so far + this batch's picks, and room for the real appends that follow it
    const int want = Q.nreal + q + 8 < QEI_MAXQ ? Q.nreal + q + 8 : QEI_MAXQ;
    if (want > Q.chain_rows) {
        if (Q.nreal > 0) {                                 // grow, keeping the real entries
            ScratchBuf keep(g->prm.device, s);
            HIPCHK(keep.b.ensure(sizeof(double) * (size_t)Q.nreal * Mp));
            HIPCHK(hipMemcpyAsync(keep.b.p, c->qchain.p, sizeof(double) * (size_t)Q.nreal * Mp, hipMemcpyDeviceToDevice, s));
            HIPCHK(wait_stream(s));
            HIPCHK(c->qchain.ensure(sizeof(double) * (size_t)want * Mp));
            HIPCHK(hipMemcpyAsync(c->qchain.p, keep.b.p, sizeof(double) * (size_t)Q.nreal * Mp, hipMemcpyDeviceToDevice, s));
        } else {
            HIPCHK(c->qchain.ensure(sizeof(double) * (size_t)want * Mp));
        }
        Q.chain_rows = want;
    }
    const QeiWork w = qei_carve(nullptr, T16, g->d, g->dp, (int)g->Np);
    HIPCHK(c->qwork.ensure(w.bytes));
    // snapshot of the stored posterior, in buffers of its own (the caller's abo_cand_save snapshot stays what it is): the batch is
    // rolled back at _end
    const size_t bytes = sizeof(double) * (c->M > 0 ? c->M : 1);
    HIPCHK(c->qmu.ensure(bytes));
    HIPCHK(c->qvar.ensure(bytes));
    if (snapshot) {                                        // (the device pick loop takes the snapshot in its first launch)
        HIPCHK(hipMemcpyAsync(c->qmu.p, c->mu.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(c->qvar.p, c->var.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, s));
    }
    // the fantasies of the last batch go; blocks and real entries stay
    Q.nchain = Q.nreal;
    Q.chain_x.resize((size_t)Q.nreal * c->d);
    Q.chain_s.resize(Q.nreal);
    Q.open = true; Q.qmax = q; Q.batch0 = Q.nreal; Q.stats = QeiBatchStats{};
    return ABO_OK;
}

// EI over the shard, its k best as records in DEVICE memory rec_d (k × (4 + d + picks so far) doubles); nothing is waited for
int32_t abo::qei_top(abo_gp* g, abo_cand* c, double xi, double best_y, int64_t idx_base, int k, double* rec_d) {
    if (!g || !c || !rec_d) return fail(ABO_EINVAL, "abo_cand_qei_top: null argument");
    if (!c->qei.open || c->qei.gen != g->st->gen || c->qei.N + c->qei.nreal != g->N) return fail(ABO_EINVAL, "abo_cand_qei_top: no batch open on this model (abo_cand_qei_begin)");
    if (k < 1 || k > 1024) return fail(ABO_EINVAL, "abo_cand_qei_top: k = %d outside 1..1024", k);
    if (int32_t r = qei_rebase(c, idx_base)) return r;
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    HIPCHK(c->score.ensure(sizeof(double) * (c->M > 0 ? c->M : 1)));
    HIPCHK(c->top_val.ensure(sizeof(double) * k));
    HIPCHK(c->top_idx.ensure(sizeof(int64_t) * k));
    HIPCHK(launch_score(c->mu.as<double>(), c->var.as<double>(), c->score.as<double>(), c->M, ABO_ACQ_EI, xi, best_y, s));
    int32_t rc = cand_topk(g, c, c->score.as<double>(), k, idx_base, c->top_val.as<double>(), c->top_idx.as<int64_t>(), ABO_DEVICE);
    if (rc) return rc;
    HIPCHK(launch_qei_record(c->top_val.as<double>(), c->top_idx.as<int64_t>(), k, idx_base, c->Z.as<double>(), c->mu.as<double>(),
                             c->var.as<double>(), c->qchain.as<double>(), c->qei.Mp, c->qei.nchain, c->d, rec_d, s));
    return ABO_OK;
}

// Cov₀(z, p_t) of T points for every candidate of the shard: K⁻¹K_XT by two split-k products against L⁻¹ / L⁻ᵀ, ONE product over the
// resident K_ZX, the kernel values k(z, p_t) on top.  pts: T × d HOST doubles, gidx their global candidate indices.
int32_t abo::qei_block(abo_gp* g, abo_cand* c, const double* pts, const int64_t* gidx, int T) {
    if (!g || !c || !pts || !gidx) return fail(ABO_EINVAL, "abo_cand_qei_block: null argument");
    abo_cand::Qei& Q = c->qei;
    if (!Q.open || Q.gen != g->st->gen || Q.N + Q.nreal != g->N) return fail(ABO_EINVAL, "abo_cand_qei_block: no batch open on this model (abo_cand_qei_begin)");
    if (T < 1 || T > Q.T16) return fail(ABO_EINVAL, "abo_cand_qei_block: T = %d outside 1..%d", T, Q.T16);
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    const int T16 = Q.T16, d = g->d, dp = g->dp, N = (int)g->N, Np = (int)g->Np;
    const int64_t ld = g->st->cap, Mp = Q.Mp;
    const int blk = Q.next_blk;
    Q.next_blk = (Q.next_blk + 1) % Q.nblk_cap;
    for (int t = 0; t < T16; ++t) Q.slot_gidx[(size_t)blk * T16 + t] = t < T ? gidx[t] : -1;
    memcpy(&Q.slot_x[(size_t)blk * T16 * g->d], pts, sizeof(double) * (size_t)T * g->d);
    Q.blk_base[blk] = Q.nreal;                             // the model of this build holds the real entries so far: they are in its columns
    ++Q.stats.builds;
    if (c->M == 0) return ABO_OK;
    const QeiWork w = qei_carve(c->qwork.p, T16, d, dp, Np);
    double* C = c->qblk.as<double>() + (size_t)blk * T16 * Mp;
    HIPCHK(g->events(EV_BASE + 4));
    hipEvent_t* ev = &g->evs()[EV_BASE];          // scratch slots: ev[0] / ev[3] the block build, ev[1] / ev[2] its pass over the set (no posterior pass in this call)
    HIPCHK(hipEventRecord(ev[0], s));
    HIPCHK(hipMemsetAsync(w.P, 0, sizeof(double) * (size_t)T16 * d, s));
    HIPCHK(hipMemcpyAsync(w.P, pts, sizeof(double) * (size_t)T * d, hipMemcpyHostToDevice, s));
    HIPCHK(launch_scale_points(w.P, w.Ps, T, T16, d, dp, 1.0 / g->prm.ell, s));
    HIPCHK(launch_qei_kxt(g->st->Xs.as<double>(), dp, N, Np, w.P, d, T, T16, g->prm.family, 1.0 / g->prm.ell, g->prm.sigma_f2, w.KXT, s));
    // V[t][i] = Σ_{k ≤ i} K_XT[t][k]·W[i][k] = (L⁻¹k_t)[i];  U[t][i] = Σ_{k ≥ i} V[t][k]·WT[i][k] = (K⁻¹k_t)[i]
    const bool via_skinny = getenv("ABO_QEI_PASS_SKINNY") != nullptr;      // A/B runs and the bit-equality test: gemm.hip's split-k kernel
    const int64_t sC = (int64_t)T16 * Np;
    GemmArgs g1{};
    g1.A = w.KXT; g1.lda = Np; g1.B = g->st->W.as<double>(); g1.ldb = ld; g1.C = w.Ct; g1.ldc = Np; g1.sC = sC;
    g1.M = TB; g1.N = Np; g1.K = Np; g1.kmode = K_B_LOWER; g1.lower_only = 0; g1.batch = 1; g1.alpha = 1.0; g1.beta = 0.0;
    g1.ksplit = w.ks; g1.mrows = T16;
    if (via_skinny) HIPCHK(launch_gemm_nt(g1, s));
    else HIPCHK(launch_qei_pass(w.KXT, Np, T16, g->st->W.as<double>(), ld, Np, Np, 1.0, w.Ct, Np, s, K_B_LOWER, w.ks, sC));
    HIPCHK(launch_splitk_reduce(w.Ct, Np, sC, w.nz, T16, Np, Np, w.ks, K_B_LOWER, w.V, Np, s));
    HIPCHK(launch_qei_zero_tail(w.V, Np, N, Np, T16, s));      // rows ≥ N of a shared factor may hold a discarded appended branch
    GemmArgs g2 = g1;
    g2.A = w.V; g2.B = g->st->WT.as<double>(); g2.kmode = K_B_UPPER;
    if (via_skinny) HIPCHK(launch_gemm_nt(g2, s));
    else HIPCHK(launch_qei_pass(w.V, Np, T16, g->st->WT.as<double>(), ld, Np, Np, 1.0, w.Ct, Np, s, K_B_UPPER, w.ks, sC));
    HIPCHK(launch_splitk_reduce(w.Ct, Np, sC, w.nz, T16, Np, Np, w.ks, K_B_UPPER, w.U, Np, s));
    HIPCHK(launch_qei_zero_tail(w.U, Np, N, Np, T16, s));
    // C[t][z] = −Σ_k U[t][k]·K_ZX[z][k]: one pass over the resident K_ZX for all T columns (columns ≥ N of K_ZX meet U = 0)
    HIPCHK(hipEventRecord(ev[1], s));
    if (via_skinny) {
        GemmArgs g3{};
        g3.A = w.U; g3.lda = Np; g3.B = c->Kzx.as<double>(); g3.ldb = c->kzx_ld; g3.C = C; g3.ldc = Mp; g3.sC = 0;
        g3.M = TB; g3.N = (int)Mp; g3.K = Np; g3.kmode = K_FULL; g3.lower_only = 0; g3.batch = 1; g3.alpha = -1.0; g3.beta = 0.0;
        g3.ksplit = Np; g3.mrows = T16;
        HIPCHK(launch_gemm_nt(g3, s));
    } else {
        HIPCHK(launch_qei_pass(w.U, Np, T16, c->Kzx.as<double>(), c->kzx_ld, Mp, Np, -1.0, C, Mp, s));
    }
    HIPCHK(hipEventRecord(ev[2], s));
    HIPCHK(launch_qei_cov(w.Ps, dp, c->Z.as<double>(), c->M, Mp, d, T, g->prm.family, 1.0 / g->prm.ell, g->prm.sigma_f2, C, s));
    HIPCHK(hipEventRecord(ev[3], s));
    HIPCHK(wait_stream(s));                          // (pts is the caller's; the events are read)
    Q.stats.block_ms += ev_ms(ev[0], ev[3]);
    Q.stats.pass_ms = ev_ms(ev[1], ev[2]);
    Q.stats.pass_bytes = 8.0 * (double)g->N * (double)c->M;
    Q.stats.pass_flop = 2.0 * (double)g->N * (double)c->M * (double)T16;
    return ABO_OK;
}

int abo::qei_block_default() { return qei_default_block(); }

size_t abo::qei_max_words(int d, int q, int T) {
    if (T <= 0) T = qei_default_block();
    if (T > QEI_MAXT) T = QEI_MAXT;
    if (T < 1) T = 1;
    (void)q;
    return (size_t)T * (size_t)(4 + d + QEI_MAXQ);        // a record carries one value per chain entry: real ones carried over + the batch's
}

int32_t abo::qei_has(const abo_cand* c, int64_t gidx) { return c && qei_find_slot(c, gidx) >= 0 ? 1 : 0; }

// condition the shard's stored variance on the pick `gidx` (a point of a block): chain vector n + 1, σ² −= c²/s with
// s = var_x + σ²_n (var_x: the stored σ² at the pick, from the winner's record), γ_i = cx[i]/s_i (cx: c_1(x) … c_n(x) from the same
// record).  s ≤ 0 is what the plain loop's bordered append reports as a failed pivot: ABO_ENOTPD, *info = N + n + 1.
int32_t abo::qei_pick(abo_gp* g, abo_cand* c, int64_t gidx, double var_x, const double* cx, int n, int64_t excl, int64_t* info) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    if (info) *info = 0;
    if (!g || !c || (n > 0 && !cx)) return fail(ABO_EINVAL, "abo_cand_qei_pick: null argument");
    abo_cand::Qei& Q = c->qei;
    if (!Q.open || Q.gen != g->st->gen || Q.N + Q.nreal != g->N) return fail(ABO_EINVAL, "abo_cand_qei_pick: no batch open on this model (abo_cand_qei_begin)");
    if (n != Q.nchain) return fail(ABO_EINVAL, "abo_cand_qei_pick: %d chain values for a chain of %d picks", n, Q.nchain);
    if (Q.nchain - Q.batch0 >= Q.qmax || Q.nchain >= Q.chain_rows) return fail(ABO_EINVAL, "abo_cand_qei_pick: the batch was opened for %d picks", Q.qmax);
    if (excl >= c->M) return fail(ABO_EINVAL, "abo_cand_qei_pick: exclusion index %lld outside the shard", (long long)excl);
    const int slot = qei_find_slot(c, gidx);
    if (slot < 0) return fail(ABO_EINVAL, "abo_cand_qei_pick: candidate %lld is in no block (abo_cand_qei_block)", (long long)gidx);
    const double sj = var_x + g->st->noise_used;
    if (!(sj > 0.0)) {
        const long long at = (long long)(g->N + (Q.nchain - Q.nreal) + 1);
        if (info) *info = at;
        return fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld", at);
    }
    HIPCHK(hipSetDevice(g->prm.device));
    hipStream_t s = g->stream;
    QeiPickArgs a{};
    a.blk = c->qblk.as<double>() + (size_t)slot * Q.Mp;
    a.chain = c->qchain.as<double>();
    a.out = c->qchain.as<double>() + (size_t)Q.nchain * Q.Mp;
    a.var = c->var.as<double>();
    a.M = c->M; a.Mp = Q.Mp; a.nchain = Q.nchain; a.s = sj;
    a.first = Q.blk_base[slot / Q.T16];                    // entries before it are already in the block's columns
    for (int i = 0; i < n; ++i) a.gam[i] = cx[i] / Q.chain_s[i];
    HIPCHK(launch_qei_pick(a, s));
    if (excl >= 0) {
        const double ex[2] = {HUGE_VAL, 0.0};                // abo_cand_exclude: μ = +Inf, σ² = 0
        HIPCHK(hipMemcpyAsync(c->mu.as<double>() + excl, &ex[0], sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c->var.as<double>() + excl, &ex[1], sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHK(wait_stream(s));                      // (ex lives on this frame)
    }
    ++Q.nchain;
    Q.chain_s.push_back(sj);
    Q.chain_x.insert(Q.chain_x.end(), &Q.slot_x[(size_t)slot * c->d], &Q.slot_x[(size_t)slot * c->d] + c->d);
    return ABO_OK;
}

int32_t abo::qei_end(abo_gp* g, abo_cand* c) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_qei_end: null argument");
    if (!c->qei.open) return ABO_OK;
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(hipMemcpyAsync(c->mu.p, c->qmu.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(c->var.p, c->qvar.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(wait_stream(g->stream));
    c->qei.open = false;
    return ABO_OK;
}

void abo::qei_get_stats(const abo_cand* c, int picks, double total_ms, abo_qei_stats* out) {
    if (!out) return;
    const abo_cand::Qei& Q = c->qei;
    const QeiBatchStats& st = Q.stats;
    const int cond = Q.nchain - Q.batch0;                                  // picks of the batch that were conditioned on
    out->picks = picks; out->block = Q.T16; out->block_builds = st.builds;
    out->block_hits = cond > st.builds ? cond - st.builds : 0;             // each of them either found its point in a block or had one built
    out->total_ms = total_ms; out->block_ms = st.block_ms; out->pass_ms = st.pass_ms; out->pass_bytes = st.pass_bytes; out->pass_flop = st.pass_flop;
}

// A new block around the current scores: the best Tk candidates over all shards (the pick `gidx` is the first of them), their
// covariance columns from ONE pass over every shard's K_ZX.  words = 4 + d + chain entries (the width of a record right now).
static int32_t qei_build_block(const abo::QeiShards& S, double xi, double best_y, int Tk, int words, int64_t gidx) {
    const int n = S.n, d = gp_dim(S.gp[0]);
    const int wt = Tk * words;
    int32_t rc = S.run([&](int i) -> int32_t { return abo::qei_top(S.gp[i], S.cd[i], xi, best_y, S.lo[i], Tk, S.rec(i)); });
    if (rc) return rc;
    std::vector<double> blocks((size_t)n * wt);
    rc = S.gather((size_t)wt, blocks.data());
    if (rc) return rc;
    struct Ent { uint64_t key; int64_t idx; const double* r; };
    std::vector<Ent> ents;
    for (int e = 0; e < n * Tk; ++e) {
        const double* r = &blocks[(size_t)e * words];
        if (r[1] >= 0) ents.push_back({host_score_key(r[0]), (int64_t)r[1], r});
    }
    std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.key > b.key || (a.key == b.key && a.idx < b.idx); });
    const int Tb = (int)ents.size() < Tk ? (int)ents.size() : Tk;
    std::vector<double> pts((size_t)Tk * d);
    std::vector<int64_t> gix(Tk);
    bool found = false;
    for (int t = 0; t < Tb; ++t) {
        gix[t] = ents[t].idx;
        memcpy(&pts[(size_t)t * d], ents[t].r + 4, sizeof(double) * d);
        found = found || ents[t].idx == gidx;
    }
    if (!found) return fail(ABO_EINVAL, "q-EI: internal error: the pick is not among the best %d", Tb);
    return S.run([&](int i) -> int32_t { return abo::qei_block(S.gp[i], S.cd[i], pts.data(), gix.data(), Tb); });
}

// The batch on ONE handle with the pick loop on the device (qei.hip: qei_step_kernel): launch k finishes pick k − 1 (record, slot
// look-up, γ, the rank-1 correction) and selects pick k — q + 1 launches and ONE read-back per batch where qei_drive makes five launches,
// a copy and a host synchronisation per pick (the kernels of a pick total ≈ 19 µs, the host round trip made it 47: VERDICT r05).  Only
// a pick outside every block (or a failed pivot) comes back to the host early: the remaining launches return at once, the host builds
// the block and resumes.  Same picks, same values, same chain as qei_drive with one shard, bit for bit (the step calls — what
// abstractbayesopt.jl_amd/incremental.py drives — are compared with this in tests/test_gpu_incremental.py).
static int32_t qei_drive_device(abo_gp* g, abo_cand* c, int q, double xi, double best_y, int distinct, int T, int64_t idx_base,
                                double* x_out, int64_t* idx_out, double* ei_out, int64_t* info) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    if (T <= 0) T = qei_default_block();
    if (T > QEI_MAXT) T = QEI_MAXT;
    const int d = c->d;
    const int Tk = (int64_t)T < c->M ? T : (int)c->M;
    int32_t rc = abo::qei_begin(g, c, q, T, /*snapshot=*/false);
    if (rc) return rc;
    abo_cand::Qei& Q = c->qei;
    hipStream_t s = g->stream;
    FirstError keep;
    bool launched = false, restored = false;               // launch 0 snapshots (μ, σ²), the tail launch rolls them back
    const int wmax = 4 + d + QEI_MAXQ;
    const size_t off_part = (sizeof(QeiStepState) + 255) / 256 * 256;
    const size_t off_rec = off_part + sizeof(QeiStepPartial) * 2 * QEI_STEP_MAXWG;
    const size_t rec_bytes = sizeof(double) * (size_t)q * wmax;
    std::vector<double> rec((size_t)q * wmax);
    QeiStepState hst{};
    do {
        if ((rc = qei_rebase(c, idx_base))) break;
        hipError_t e = c->qdev.ensure(off_rec + rec_bytes);
        if (e == hipSuccess) e = hipMemsetAsync(c->qdev.p, 0, sizeof(QeiStepState), s);
        if (e != hipSuccess) { rc = fail(ABO_EHIP, "abo_cand_qei: %s", hipGetErrorString(e)); break; }
        char* base = static_cast<char*>(c->qdev.p);
        QeiStepArgs a{};
        a.mu = c->mu.as<double>(); a.var = c->var.as<double>(); a.Z = c->Z.as<double>();
        a.snap_mu = c->qmu.as<double>(); a.snap_var = c->qvar.as<double>();
        a.blk = c->qblk.as<double>(); a.chain = c->qchain.as<double>();
        a.st = reinterpret_cast<QeiStepState*>(base);
        a.part = reinterpret_cast<QeiStepPartial*>(base + off_part);
        a.rec = reinterpret_cast<double*>(base + off_rec);
        a.M = c->M; a.Mp = Q.Mp; a.idx_base = idx_base; a.d = d; a.T16 = Q.T16; a.nslots = Q.nblk_cap * Q.T16; a.wmax = wmax;
        a.q = q; a.n0 = Q.nchain; a.distinct = distinct; a.xi = xi; a.best_y = best_y; a.noise = g->st->noise_used;
        for (int i = 0; i < Q.nchain; ++i) a.chain_s0[i] = Q.chain_s[i];
        const int nwg = (int)std::min<int64_t>((c->M + 255) / 256, QEI_STEP_MAXWG);
        a.nwg_prev = nwg;
        int k_from = 0, done = 0;                              // done: picks of the batch the chain holds already
        while (true) {
            for (int b = 0; b < 4; ++b) a.blk_base[b] = b < Q.nblk_cap ? Q.blk_base[b] : 0;
            for (int e2 = 0; e2 < 4 * QEI_MAXT; ++e2) a.slot_gidx[e2] = e2 < a.nslots ? Q.slot_gidx[e2] : -1;
            for (int k = k_from; k <= q && e == hipSuccess; ++k) { a.k = k; e = launch_qei_step(a, nwg, s); launched = true; }
            PinStage pin(g->ctx);
            if (e == hipSuccess) e = pin.d2h(&hst, a.st, sizeof(QeiStepState), s);
            if (e == hipSuccess) e = pin.d2h(rec.data(), a.rec, rec_bytes, s);
            if (e == hipSuccess) e = wait_stream(s);
            if (e != hipSuccess) { rc = fail(ABO_EHIP, "abo_cand_qei: %s", hipGetErrorString(e)); break; }
            pin.flush();
            // the picks conditioned on since the last read-back join the host's image of the chain (abo_cand_downdate compares a real
            // append's point with chain_x to find its column)
            const int cond = hst.stop ? hst.stop_at : q - 1;
            for (int t = done; t < cond; ++t) {
                const double* r = &rec[(size_t)t * wmax];
                ++Q.nchain;
                Q.chain_s.push_back(hst.s_batch[t]);
                Q.chain_x.insert(Q.chain_x.end(), r + 4, r + 4 + d);
            }
            done = cond;
            if (!hst.stop) { restored = true; break; }    // the tail launch ran: the stored posterior is the batch's starting point again
            const double* r = &rec[(size_t)hst.stop_at * wmax];
            if (hst.stop == 2) {                               // s = σ²(x) + σ²_n ≤ 0: the failed pivot of the plain loop's bordered append
                const long long at = (long long)(g->N + (Q.nchain - Q.nreal) + 1);
                if (info) *info = at;
                rc = fail(ABO_ENOTPD, "PosDefException: matrix is not positive definite; Cholesky factorization failed at %lld", at);
                break;
            }
            // pick stop_at lies in no block: a new block around the scores of this moment, then the launches from stop_at + 1 again
            const OneShard one(g, c, idx_base);
            if ((rc = qei_build_block(one.S, xi, best_y, Tk, 4 + d + Q.nchain, (int64_t)r[1]))) break;
            e = hipMemsetAsync(&a.st->stop, 0, 2 * sizeof(int32_t), s);
            k_from = hst.stop_at + 1;
        }
        if (rc) break;
        for (int j = 0; j < q; ++j) {
            const double* r = &rec[(size_t)j * wmax];
            ei_out[j] = r[0];
            idx_out[j] = (int64_t)r[1];
            memcpy(x_out + (size_t)j * d, r + 4, sizeof(double) * d);
        }
    } while (false);
    keep.note(rc);
    int32_t r2 = ABO_OK;
    if (restored || !launched) c->qei.open = false;        // nothing to roll back (or nothing was touched)
    else r2 = abo::qei_end(g, c);                          // an error after launch 0: σ², μ back from the snapshot it took
    return rc ? keep.report(rc) : r2;
}

// The batch over n shards of one set.  S.run(f): f(i) on every shard (mgpu: the shard's worker thread); S.rec(i): the shard's
// record block in DEVICE memory (room for S.max_words doubles); S.gather(words, out): all shards' blocks → host, n × words doubles.
int32_t abo::qei_drive(const QeiShards& S, int q, double xi, double best_y, int distinct, int T, double* x_out, int64_t* idx_out,
                       double* ei_out, int64_t* info) {
    const int n = S.n, d = gp_dim(S.gp[0]);
    if (T <= 0) T = qei_default_block();
    if (T > QEI_MAXT) T = QEI_MAXT;
    int64_t Mtot = 0;
    for (int i = 0; i < n; ++i) Mtot += S.cd[i]->M;
    if (Mtot < 1) return fail(ABO_EINVAL, "q-EI: the candidate set is empty");
    const int Tk = (int64_t)T < Mtot ? T : (int)Mtot;
    int32_t rc = S.run([&](int i) -> int32_t { return abo::qei_begin(S.gp[i], S.cd[i], q, T); });
    FirstError keep;
    keep.note(rc);
    std::vector<double> blocks;
    int nch_done = rc ? 0 : S.cd[0]->qei.nchain;           // the real entries the state carries over
    for (int j = 0; j < q && !rc; ++j) {
        const int nch = nch_done, words = 4 + d + nch;
        rc = S.run([&](int i) -> int32_t { return abo::qei_top(S.gp[i], S.cd[i], xi, best_y, S.lo[i], 1, S.rec(i)); });
        if (rc) break;
        blocks.resize((size_t)n * words);
        rc = S.gather((size_t)words, blocks.data());
        if (rc) break;
        int win = -1;
        for (int i = 0; i < n; ++i) {                          // sortperm(scores; rev=true)[1] over the shards' winners
            const double* r = &blocks[(size_t)i * words];
            if (r[1] < 0) continue;                            // empty shard
            if (win < 0) { win = i; continue; }
            const double* w = &blocks[(size_t)win * words];
            const uint64_t kr = host_score_key(r[0]), kw = host_score_key(w[0]);
            if (kr > kw || (kr == kw && r[1] < w[1])) win = i;
        }
        if (win < 0) { rc = fail(ABO_EINVAL, "q-EI: the candidate set is empty"); break; }
        const std::vector<double> w(blocks.begin() + (size_t)win * words, blocks.begin() + (size_t)(win + 1) * words);
        const int64_t gidx = (int64_t)w[1];
        ei_out[j] = w[0];
        idx_out[j] = gidx;
        memcpy(x_out + (size_t)j * d, &w[4], sizeof(double) * d);
        if (j == q - 1) break;                                 // the last pick conditions nothing (the batch is rolled back)
        if (!abo::qei_has(S.cd[0], gidx)) {
            rc = qei_build_block(S, xi, best_y, Tk, words, gidx);
            if (rc) break;
        }
        rc = S.run([&](int i) -> int32_t {
            const int64_t ex = (distinct && gidx >= S.lo[i] && gidx < S.lo[i] + S.cd[i]->M) ? gidx - S.lo[i] : -1;
            int64_t inf = 0;
            const int32_t r = abo::qei_pick(S.gp[i], S.cd[i], gidx, w[3], &w[4 + d], nch, ex, &inf);
            if (inf && info && i == 0) *info = inf;
            return r;
        });
        if (rc) break;
        ++nch_done;
    }
    keep.note(rc);
    const int32_t r2 = S.run([&](int i) -> int32_t { return abo::qei_end(S.gp[i], S.cd[i]); });
    return rc ? keep.report(rc) : r2;
}

// The Monte-Carlo joint q-EI (qei_mc.hip) on the set's block state: the continuation rule of qei_begin, but the chain (real entries and
// the last batch's fantasies) is only read, and another block size re-keys the ring instead of dropping the chain.
int32_t abo::qei_mc_open(abo_gp* g, abo_cand* c, int q, int T, int64_t idx_base, QeiBatchStats* keep) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    int32_t rc = check_fitted(g, c->d);
    if (rc) return rc;
    if (g->p_out > 1) return fail(ABO_EINVAL, "abo_cand_qei_mc: gradient-enhanced models are not supported (a standard GP only)");
    if (c->M > 0 && !c->resident(g))
        return fail(ABO_EINVAL, "abo_cand_qei_mc: K_ZX of the set is not resident (ABO_CAND_KZX_GIB): the Monte-Carlo q-EI reads its blocks from it");
    if (g->prm.device != c->device) return fail(ABO_EINVAL, "abo_cand_qei_mc: candidate set lives on device %d, model on %d", c->device, g->prm.device);
    if (!c->in_sync(g))
        return fail(ABO_EINVAL, "abo_cand_qei_mc: the candidate set is not in sync with this model (abo_cand_refresh / abo_cand_downdate)");
    if ((size_t)QEI_MAXT * c->d * sizeof(double) > 65536) return fail(ABO_EINVAL, "abo_cand_qei_mc: d = %d > 128 (a block's points fill LDS)", c->d);
    if (T > QEI_MAXT) T = QEI_MAXT;
    HIPCHK(hipSetDevice(g->prm.device));
    abo_cand::Qei& Q = c->qei;
    const int T16 = (int)pad_up(T, 16);
    const int64_t Mp = pad_up(c->M > 0 ? c->M : 1, TB);
    if ((rc = qei_open_state(g, c, T16, Mp, 0, /*rekey=*/true))) return rc;
    HIPCHK(c->qblk.ensure(sizeof(double) * (size_t)Q.nblk_cap * T16 * Mp));
    HIPCHK(c->qwork.ensure(qei_carve(nullptr, T16, g->d, g->dp, (int)g->Np).bytes));
    if ((rc = qei_rebase(c, idx_base))) return rc;
    *keep = Q.stats;
    Q.stats = QeiBatchStats{};
    Q.open = true;
    return ABO_OK;
}

void abo::qei_mc_view(abo_cand* c, QeiMcView* v) {
    const abo_cand::Qei& Q = c->qei;
    v->mu = c->mu.as<double>(); v->var = c->var.as<double>(); v->Z = c->Z.as<double>();
    v->blk = c->qblk.as<double>(); v->chain = c->qchain.as<double>();
    v->M = c->M; v->Mp = Q.Mp; v->d = c->d; v->T16 = Q.T16; v->nslots = Q.nblk_cap * Q.T16; v->nreal = Q.nreal;
    v->blk_base = Q.blk_base.data(); v->slot_gidx = Q.slot_gidx.data(); v->chain_s = Q.chain_s.data();
    v->now = Q.stats;
}

void abo::qei_mc_close(abo_cand* c, const QeiBatchStats& keep) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    c->qei.open = false;
    c->qei.stats = keep;
}

extern "C" {

// ---- greedy q-EI on one handle (include/abo_hip.h: "block form") ----------------------------------------------------------------
int32_t abo_set_qei_block(int32_t block) {
    if (block < 0 || block > QEI_MAXT) return fail(ABO_EINVAL, "abo_set_qei_block: block = %d outside 0..%d", block, QEI_MAXT);
    g_qei_block.store(block);
    return ABO_OK;
}

int32_t abo_cand_qei_begin(abo_gp* g, abo_cand* c, int32_t q, int32_t block) { return abo::qei_begin(g, c, q, block); }

int32_t abo_cand_qei_eligible(abo_gp* g, abo_cand* c, int32_t q, int32_t block, int32_t* ok) {
    if (!g || !c || !ok) return fail(ABO_EINVAL, "abo_cand_qei_eligible: null argument");
    const int T = block <= 0 ? qei_default_block() : block;
    *ok = 0;
    if (T < 1) { (void)fail(ABO_EINVAL, "q-EI, block form: block size 0 (the plain loop is a different call)"); return ABO_OK; }
    *ok = abo::qei_eligible(g, c, q) == ABO_OK ? 1 : 0;                                   // (the reason stays in abo_last_error)
    return ABO_OK;
}

int32_t abo_cand_qei_top(abo_gp* g, abo_cand* c, double xi, double best_y, int64_t idx_base, int32_t k, double* rec, int64_t cap_words) {
    if (!g || !c || !rec) return fail(ABO_EINVAL, "abo_cand_qei_top: null argument");
    if (k < 1 || k > 1024) return fail(ABO_EINVAL, "abo_cand_qei_top: k = %d outside 1..1024", k);
    const size_t words = (size_t)k * (4 + c->d + c->qei.nchain);
    if (cap_words < 0 || (size_t)cap_words < words)
        return fail(ABO_EINVAL, "abo_cand_qei_top: rec holds %lld doubles, %d records of 4 + d + %d chain values need %zu", (long long)cap_words, k,
                    c->qei.nchain, words);
    HIPCHK(hipSetDevice(g->prm.device));
    HIPCHK(c->qrec.ensure(sizeof(double) * words));
    int32_t rc = abo::qei_top(g, c, xi, best_y, idx_base, k, c->qrec.as<double>());
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(rec, c->qrec.p, sizeof(double) * words, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(wait_stream(g->stream));
    return ABO_OK;
}

int32_t abo_cand_qei_block(abo_gp* g, abo_cand* c, const double* pts, const int64_t* gidx, int32_t T) {
    return abo::qei_block(g, c, pts, gidx, T);
}

int32_t abo_cand_qei_pick(abo_gp* g, abo_cand* c, int64_t gidx, double var_x, const double* cx, int32_t n, int64_t excl, int64_t* info) {
    return abo::qei_pick(g, c, gidx, var_x, cx, n, excl, info);
}

int32_t abo_cand_qei_end(abo_gp* g, abo_cand* c) { return abo::qei_end(g, c); }

int32_t abo_cand_qei_has(abo_gp* g, abo_cand* c, int64_t gidx, int32_t* has, int32_t* nchain) {
    if (!g || !c) return fail(ABO_EINVAL, "abo_cand_qei_has: null argument");
    if (has) *has = (c->qei.N >= 0 && gidx >= 0) ? abo::qei_has(c, gidx) : 0;
    if (nchain) *nchain = c->qei.N >= 0 ? c->qei.nchain : 0;
    return ABO_OK;
}

int32_t abo_cand_qei_stats(abo_gp* g, abo_cand* c, abo_qei_stats* out) {
    if (!g || !c || !out) return fail(ABO_EINVAL, "abo_cand_qei_stats: null argument");
    abo::qei_get_stats(c, c->qei.nchain - c->qei.batch0 + 1, 0.0, out);
    return ABO_OK;
}

// the plain loop on one handle: q × [EI + arg-max, fantasy append, O(N·M) down-date], rolled back (what abo_mgpu_cand_qei's plain
// loop does per device)
static int32_t qei_plain(abo_gp* g, abo_cand* c, int q, double xi, double best_y, int distinct, int64_t idx_base, double* x_out,
                         int64_t* idx_out, double* ei_out, int64_t* info) {
    if (c) ++c->mu_epoch;                                  // (the resident sample-path selection re-reads the exclusions)
    int32_t rc = check_fitted(g, c->d);
    if (rc) return rc;
    if (!c->in_sync(g))
        return fail(ABO_EINVAL, "abo_cand_qei: the candidate set is not in sync with this model (abo_cand_refresh / abo_cand_downdate)");
    HIPCHK(hipSetDevice(g->prm.device));
    const int d = c->d;
    const size_t bytes = sizeof(double) * (c->M > 0 ? c->M : 1);
    HIPCHK(c->qmu.ensure(bytes));
    HIPCHK(c->qvar.ensure(bytes));
    HIPCHK(hipMemcpyAsync(c->qmu.p, c->mu.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(c->qvar.p, c->var.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream));
    HIPCHK(wait_stream(g->stream));
    const uint64_t gen0 = c->synced_gen;
    const int64_t N0 = c->synced_N;
    c->qei = abo_cand::Qei();
    abo_gp* cur = g;
    FirstError keep;
    for (int j = 0; j < q && !rc; ++j) {
        double tv = 0.0, mu = 0.0;
        int64_t ti = -1;
        rc = abo::cand_acq_ex(cur, c, ABO_ACQ_EI, xi, best_y, idx_base, nullptr, ABO_DEVICE, 1, &tv, &ti, ABO_HOST);
        if (rc) break;
        if (ti < 0) { rc = fail(ABO_EINVAL, "abo_cand_qei: the candidate set is empty"); break; }
        double* x = x_out + (size_t)j * d;
        rc = abo_cand_point(cur, c, ti - idx_base, x, &mu, nullptr);
        if (rc) break;
        ei_out[j] = tv; idx_out[j] = ti;
        if (j == q - 1) break;
        abo_gp* nw = nullptr;
        if (cur->p_out > 1) {
            double yv[MAX_P];
            rc = abo_predict_grad(cur, x, 1, d, ABO_HOST, yv, nullptr, ABO_HOST);
            if (!rc) rc = abo_append_grad(cur, x, d, yv, info, &nw);
        } else {
            rc = abo_append(cur, x, d, mu, info, &nw);
        }
        if (rc) break;
        rc = abo_cand_downdate(nw, c);
        if (!rc && distinct) rc = abo_cand_exclude(nw, c, ti - idx_base);
        if (cur != g) abo_destroy(cur);
        cur = nw;
    }
    keep.note(rc);
    if (cur != g) abo_destroy(cur);
    hipError_t e = hipMemcpyAsync(c->mu.p, c->qmu.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->var.p, c->qvar.p, sizeof(double) * c->M, hipMemcpyDeviceToDevice, g->stream);
    if (e == hipSuccess) e = wait_stream(g->stream);
    c->synced_gen = gen0; c->synced_N = N0;
    if (rc) return keep.report(rc);
    HIPCHK(e);
    return ABO_OK;
}

int32_t abo_cand_qei(abo_gp* g, abo_cand* c, int32_t q, double xi, double best_y, int32_t distinct, int64_t idx_base, int32_t block,
                     double* x_out, int64_t* idx_out, double* ei_out, abo_qei_stats* stats) {
    if (!g || !c || !x_out || !idx_out || !ei_out) return fail(ABO_EINVAL, "abo_cand_qei: null argument");
    if (q < 1) return fail(ABO_EINVAL, "abo_cand_qei: q = %d", q);
    const auto t0 = std::chrono::steady_clock::now();
    int64_t info = 0;
    int T = block == 0 ? qei_default_block() : block;
    int32_t rc;
    if (T > 0 && abo::qei_eligible(g, c, q) == ABO_OK) {
        HIPCHK(hipSetDevice(g->prm.device));
        HIPCHK(c->qrec.ensure(sizeof(double) * abo::qei_max_words(c->d, q, T)));
        // one handle, at least one candidate: the pick loop stays on the device; an empty set goes through the shard driver (its
        // "the candidate set is empty" is the contract)
        if (c->M >= 1) rc = qei_drive_device(g, c, q, xi, best_y, distinct, T, idx_base, x_out, idx_out, ei_out, &info);
        else rc = abo::qei_drive(OneShard(g, c, idx_base).S, q, xi, best_y, distinct, T, x_out, idx_out, ei_out, &info);
    } else {
        (void)hipGetLastError();
        rc = qei_plain(g, c, q, xi, best_y, distinct, idx_base, x_out, idx_out, ei_out, &info);
    }
    if (stats) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        abo::qei_get_stats(c, q, ms, stats);
    }
    return rc;
}

}  // extern "C"
