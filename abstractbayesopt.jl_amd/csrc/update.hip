// abo_update / abo_mgpu_update (include/abo_hip.h): update(model, xs, ys) that reuses the fitted model when (xs, ys) extends the data it
// is conditioned on — the call the reference's BO loop makes every iteration (src/bayesian_opt.jl:119-125).
//
// One device pass decides: the prefix-match kernel compares the caller's X[0:Nprev], y[0:Nprev] with the storage's Xraw / ybuf as 64-bit
// words (one flag word) and packs the k new points for the host; flag and points come back with the call's single synchronisation,
// before any append is queued.  No training data crosses to the host.  The appends themselves are api.hip's (abo_internal.h:
// gp_append_into → append_impl / append_grad_impl); every other case is the plain refit of abo_create(_grad) + abo_fit.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/abo_hip.h"
#include "abo_internal.h"

namespace abo {
namespace {

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_MAX_BLOCKS = 1024;

// Crossover rule (header: abo_update): k·p appended rows against one refit of R = prev's factor rows.  Measured with
// tools/update_latency.py (profiles/update_latency.txt): break-even at k ≈ 10 for R = 1024, beyond 64 for R = 8192.
int64_t kmax_rows(int64_t R) {
    const int64_t k = R / 128;
    return k < 4 ? 4 : (k > 64 ? 64 : k);
}

// flag |= any word of the prefix differs; tail = the k new points, x_j (d words each), then their p values point-major (j·p + q).
// y is the caller's: by outputs (y[q·N + i]) for p > 1; ybuf is point-major.
__global__ void __launch_bounds__(MATCH_THREADS) prefix_match_kernel(const uint64_t* __restrict__ Xc, const uint64_t* __restrict__ yc,
                                                                      const uint64_t* __restrict__ Xraw, const uint64_t* __restrict__ ybuf,
                                                                      int64_t Nprev, int64_t N, int d, int P,
                                                                      unsigned long long* flag, uint64_t* __restrict__ tail) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nx = Nprev * d, ny = Nprev * P;
    bool bad = false;
    for (int64_t w = gid; w < nx; w += stride) bad |= Xc[w] != Xraw[w];
    if (P == 1) {
        for (int64_t w = gid; w < ny; w += stride) bad |= yc[w] != ybuf[w];
    } else {
        for (int64_t w = gid; w < ny; w += stride) {
            const int64_t i = w / P, q = w - i * P;
            bad |= yc[q * N + i] != ybuf[w];
        }
    }
    if (__ballot(bad) != 0 && __lane_id() == 0) atomicOr(flag, 1ull);
    const int64_t k = N - Nprev;
    for (int64_t t = gid; t < k * d; t += stride) tail[t] = Xc[Nprev * d + t];
    for (int64_t t = gid; t < k * P; t += stride) {
        const int64_t j = t / P, q = t - j * P;
        tail[k * d + t] = yc[q * N + Nprev + j];
    }
}

uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

// prev's parameters against the caller's, bit for bit (device only for a single handle: a group's list is its own)
bool same_params(const abo_params& a, const abo_params& b, bool device) {
    return a.family == b.family && (!device || a.device == b.device) && bits(a.ell) == bits(b.ell) && bits(a.sigma_f2) == bits(b.sigma_f2) &&
           bits(a.noise_var) == bits(b.noise_var) && bits(a.mean_c) == bits(b.mean_c) && bits(a.jitter) == bits(b.jitter);
}

// why prev cannot be extended by (N, d, params): nullptr when it can; *grow = the refit should double the capacity
const char* blocker(const GpState& ps, const abo_params& prm, const abo_params* params, const double* mean_c, int64_t N, int d,
                    bool device, bool* grow) {
    *grow = false;
    if (!ps.fitted) return "prev is not fitted";
    if (d != ps.d) return "dimension differs";
    if (N < ps.npts) return "fewer points than prev";
    if (!same_params(prm, *params, device)) return "hyper-parameters differ";
    if (ps.p_out > 1)
        for (int q = 0; q < ps.p_out; ++q)
            if (bits(ps.mean_vec[q]) != bits(mean_c ? mean_c[q] : 0.0)) return "prior means differ";
    if (bits(ps.noise_used) != bits(params->noise_var)) return "prev's factor was jittered";
    const int64_t add = (N - ps.npts) * ps.p_out;
    if (add > kmax_rows(ps.rows)) return "beyond the crossover rule";
    if (ps.rows + add > ps.cap_rows) { *grow = true; return "storage full"; }
    if (ps.max_live > ps.rows) return "another view appended past prev";
    return nullptr;
}

// The prefix match on `run`'s stream (a fresh handle on prev's device: prev itself may be in use by another thread through a copy).
// X / y: caller buffers in `space`.  On success *match says whether the prefix agrees and tail (k·(d + p) doubles) holds the new points.
int32_t prefix_match(const GpState& ps, abo_gp* run, const double* X, int64_t N, int d, const double* y, int32_t space, bool* match,
                     std::vector<double>* tail) {
    const int P = ps.p_out;
    const int64_t k = N - ps.npts;
    const size_t tail_words = (size_t)k * (d + P);
    const size_t head = 16 + sizeof(double) * tail_words;                // flag word (padded), tail
    const size_t staged = space == ABO_DEVICE ? 0 : sizeof(double) * (size_t)N * (d + P);
    hipStream_t s = gp_stream(run);
    void* buf = nullptr;
    size_t cap = 0;
    hipError_t e = scratch_alloc(ps.device, head + staged, &buf, &cap);
    if (e != hipSuccess) return set_error(e == hipErrorOutOfMemory ? ABO_ENOMEM : ABO_EHIP, "abo_update: scratch allocation failed");
    struct Release { int dev; void* p; size_t cap; hipStream_t s; ~Release() { (void)stream_wait(s); scratch_free(dev, p, cap); } }
        rel{ps.device, buf, cap, s};
    char* b = static_cast<char*>(buf);
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(b);
    double* tail_d = reinterpret_cast<double*>(b + 16);
    const double* Xd = X;
    const double* yd = y;
    if (staged) {                                                          // host inputs: staged to the device, compared there
        double* sx = reinterpret_cast<double*>(b + head);
        double* sy = sx + (size_t)N * d;
        e = hipMemcpyAsync(sx, X, sizeof(double) * (size_t)N * d, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sy, y, sizeof(double) * (size_t)N * P, hipMemcpyHostToDevice, s);
        Xd = sx; yd = sy;
    }
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return set_error(ABO_EHIP, "abo_update: staging failed");
    const int64_t words = ps.npts * (d + P) > (int64_t)tail_words ? ps.npts * (d + P) : (int64_t)tail_words;
    int64_t blocks = (words + MATCH_THREADS - 1) / MATCH_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > MATCH_MAX_BLOCKS ? MATCH_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(prefix_match_kernel, dim3((unsigned)blocks), dim3(MATCH_THREADS), 0, s,
                       reinterpret_cast<const uint64_t*>(Xd), reinterpret_cast<const uint64_t*>(yd),
                       reinterpret_cast<const uint64_t*>(ps.Xraw), reinterpret_cast<const uint64_t*>(ps.ybuf), ps.npts, N, d, P, flag,
                       reinterpret_cast<uint64_t*>(tail_d));
    e = hipGetLastError();
    if (e != hipSuccess) return set_error(ABO_EHIP, "abo_update: prefix-match launch failed");
    // flag and new points: into the page-locked block of `run` when they fit (an asynchronous copy), else straight to the host
    size_t pin_bytes = 0;
    char* pin = gp_pin(run, &pin_bytes);
    const size_t back = head;
    unsigned long long fl = 0;
    tail->assign(tail_words, 0.0);
    if (pin && back <= pin_bytes) {
        e = hipMemcpyAsync(pin, buf, back, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = stream_wait(s);
        if (e != hipSuccess) return set_error(ABO_EHIP, "abo_update: read-back failed");
        memcpy(&fl, pin, sizeof fl);
        if (tail_words) memcpy(tail->data(), pin + 16, sizeof(double) * tail_words);
    } else {
        e = hipMemcpyAsync(&fl, flag, sizeof fl, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && tail_words) e = hipMemcpyAsync(tail->data(), tail_d, sizeof(double) * tail_words, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = stream_wait(s);
        if (e != hipSuccess) return set_error(ABO_EHIP, "abo_update: read-back failed");
    }
    *match = fl == 0;
    return ABO_OK;
}

// a fresh un-conditioned handle of prev's kind
int32_t new_like(const abo_params& prm, const GpState& ps, abo_gp** out) {
    return ps.p_out > 1 ? abo_create_grad(&prm, ps.p_out, ps.mean_vec, out) : abo_create(&prm, out);
}

int32_t keep_error(int32_t rc) { const std::string t = last_error_text(); return set_error(rc, t.c_str()); }

int32_t refit(const abo_params* params, int P, const double* mean_c, const double* X, int64_t N, int d, const double* y, int32_t space,
              int64_t* info, int32_t* path, abo_gp** out, bool grow) {
    abo_params p = *params;
    if (grow && p.n_max < 2 * N) p.n_max = 2 * N;
    abo_gp* g = nullptr;
    int32_t rc = P > 1 ? abo_create_grad(&p, P, mean_c, &g) : abo_create(&p, &g);
    if (rc) return rc;
    rc = abo_fit(g, X, N, d, y, space, info);
    if (rc) { const std::string t = last_error_text(); abo_destroy(g); return set_error(rc, t.c_str()); }
    if (path) *path = ABO_UPDATE_REFIT;
    *out = g;
    return ABO_OK;
}

int32_t check_args(const char* fn, const void* prev, const abo_params* params, const double* X, int64_t N, int32_t d, const double* y,
                   int32_t space, const void* out) {
    char msg[160];
    if (!prev || !params || !X || !y || !out) { snprintf(msg, sizeof msg, "%s: null argument", fn); return set_error(ABO_EINVAL, msg); }
    if (N < 1 || N > (int64_t)1 << 20) { snprintf(msg, sizeof msg, "%s: N = %lld outside 1..2^20", fn, (long long)N); return set_error(ABO_EINVAL, msg); }
    if (d < 1 || d > 65536) { snprintf(msg, sizeof msg, "%s: input dimension %d outside 1..65536", fn, d); return set_error(ABO_EINVAL, msg); }
    if (space != ABO_HOST && space != ABO_DEVICE) { snprintf(msg, sizeof msg, "%s: unknown memory space %d", fn, space); return set_error(ABO_EINVAL, msg); }
    return ABO_OK;
}

}  // namespace
}  // namespace abo

using namespace abo;

extern "C" {

int32_t abo_update(abo_gp* prev, const abo_params* params, const double* mean_c, const double* X, int64_t N, int32_t d, const double* y,
                   int32_t space, int64_t* info, int32_t* path, abo_gp** out) {
    if (info) *info = 0;
    if (path) *path = ABO_UPDATE_REFIT;
    int32_t rc = check_args("abo_update", prev, params, X, N, d, y, space, out);
    if (rc) return rc;
    if (hipSetDevice(gp_device(prev)) != hipSuccess) return set_error(ABO_EHIP, "abo_update: hipSetDevice failed");
    GpState ps;
    gp_state(prev, &ps);
    const int P = ps.p_out;
    const abo_params prm = gp_params(prev);
    bool grow = false;
    if (blocker(ps, prm, params, mean_c, N, d, /*device=*/true, &grow))
        return refit(params, P, mean_c, X, N, d, y, space, info, path, out, grow);
    abo_gp* n = nullptr;                                       // the first appended view; its stream runs the match
    rc = new_like(prm, ps, &n);
    if (rc) return rc;
    bool match = false;
    std::vector<double> tail;
    rc = prefix_match(ps, n, X, N, d, y, space, &match, &tail);
    if (rc) { abo_destroy(n); return keep_error(rc); }
    const int64_t k = N - ps.npts;
    if (!match || k == 0) {
        abo_destroy(n);
        if (!match) return refit(params, P, mean_c, X, N, d, y, space, info, path, out, false);
        abo_retain(prev);
        if (path) *path = ABO_UPDATE_SHARED;
        *out = prev;
        return ABO_OK;
    }
    const double* tx = tail.data();
    const double* ty = tail.data() + k * d;
    abo_gp* cur = prev;
    for (int64_t j = 0; j < k; ++j) {
        if (!n) {
            rc = new_like(prm, ps, &n);
            if (rc) { if (cur != prev) abo_destroy(cur); return keep_error(rc); }
        }
        int64_t inf = 0;
        rc = gp_append_into(cur, n, tx + j * d, ty + j * P, &inf);
        const bool moved = rc == ABO_OK && gp_storage(n) != ps.storage;      // the append refitted after all (another view took the rows)
        if (cur != prev) abo_destroy(cur);
        cur = prev;
        if (rc || moved) {
            const std::string t = last_error_text();
            abo_destroy(n);
            if (rc == ABO_ENOTPD && !(params->jitter > 0.0)) {
                if (info) *info = inf;
                return set_error(rc, t.c_str());
            }
            if (rc && rc != ABO_ENOTPD) return set_error(rc, t.c_str());
            return refit(params, P, mean_c, X, N, d, y, space, info, path, out, false);
        }
        cur = n;
        n = nullptr;
    }
    if (path) *path = ABO_UPDATE_APPENDED;
    *out = cur;
    return ABO_OK;
}

int32_t abo_mgpu_update(abo_mgpu* prev, const abo_params* params, const double* mean_c, const double* X, int64_t N, int32_t d,
                        const double* y, int64_t* info, int32_t* path, abo_mgpu** out) {
    if (info) *info = 0;
    if (path) *path = ABO_UPDATE_REFIT;
    int32_t rc = check_args("abo_mgpu_update", prev, params, X, N, d, y, ABO_HOST, out);
    if (rc) return rc;
    int32_t ndev = 0, dev[16];
    rc = abo_mgpu_info(prev, &ndev, dev, nullptr);
    if (rc) return rc;
    abo_gp* g0 = nullptr;
    rc = abo_mgpu_get(prev, 0, &g0);
    if (rc) return rc;
    if (hipSetDevice(gp_device(g0)) != hipSuccess) return set_error(ABO_EHIP, "abo_mgpu_update: hipSetDevice failed");
    GpState ps;
    gp_state(g0, &ps);
    const int P = ps.p_out;
    const abo_params prm = gp_params(g0);
    auto refit_group = [&](bool grow) -> int32_t {
        abo_params p = *params;
        if (grow && p.n_max < 2 * N) p.n_max = 2 * N;
        abo_mgpu* g = nullptr;
        int32_t r = P > 1 ? abo_mgpu_create_grad(&p, P, mean_c, ndev, dev, &g) : abo_mgpu_create(&p, ndev, dev, &g);
        if (r) return r;
        r = abo_mgpu_fit(g, X, N, d, y, info);
        if (r) { const std::string t = last_error_text(); abo_mgpu_destroy(g); return set_error(r, t.c_str()); }
        if (path) *path = ABO_UPDATE_REFIT;
        *out = g;
        return ABO_OK;
    };
    bool grow = false;
    if (blocker(ps, prm, params, mean_c, N, d, /*device=*/false, &grow)) return refit_group(grow);
    // every shard has a storage of its own: each must have room and no view past prev
    std::vector<const void*> stor(ndev);
    for (int i = 0; i < ndev; ++i) {
        abo_gp* gi = nullptr;
        GpState si;
        if (abo_mgpu_get(prev, i, &gi) || !gp_state(gi, &si)) return refit_group(false);
        if (si.max_live > si.rows) return refit_group(false);
        stor[i] = si.storage;
    }
    abo_gp* run = nullptr;                                     // a handle on the first device for the match's stream
    rc = new_like(prm, ps, &run);
    if (rc) return rc;
    bool match = false;
    std::vector<double> tail;
    rc = prefix_match(ps, run, X, N, d, y, ABO_HOST, &match, &tail);
    abo_destroy(run);
    if (rc) return keep_error(rc);
    if (!match) return refit_group(false);
    const int64_t k = N - ps.npts;
    abo_mgpu* c = nullptr;
    rc = abo_mgpu_clone(prev, &c);
    if (rc) return rc;
    const double* tx = tail.data();
    const double* ty = tail.data() + k * d;
    for (int64_t j = 0; j < k; ++j) {
        int64_t inf = 0;
        rc = P > 1 ? abo_mgpu_append_grad(c, tx + j * d, d, ty + j * P, &inf, nullptr) : abo_mgpu_append(c, tx + j * d, d, ty[j], &inf, nullptr);
        bool moved = false;
        for (int i = 0; i < ndev && rc == ABO_OK; ++i) {
            abo_gp* gi = nullptr;
            moved = moved || abo_mgpu_get(c, i, &gi) != ABO_OK || gp_storage(gi) != stor[i];
        }
        if (rc || moved) {
            const std::string t = last_error_text();
            abo_mgpu_destroy(c);
            if (rc == ABO_ENOTPD && !(params->jitter > 0.0)) {
                if (info) *info = inf;
                return set_error(rc, t.c_str());
            }
            if (rc && rc != ABO_ENOTPD) return set_error(rc, t.c_str());
            return refit_group(false);
        }
    }
    if (path) *path = k == 0 ? ABO_UPDATE_SHARED : ABO_UPDATE_APPENDED;
    *out = c;
    return ABO_OK;
}

}  // extern "C"
