/* Plain-C host of abo_update (test infrastructure, run as a child process by tests/test_gpu_update.py): fit, then five
 * driver-shaped updates (the previous points plus one new one), then a posterior — checked against a refit on the same data.
 * Exit 0 and "c_update_harness ok" on success. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "abo_hip.h"

#define N0 160
#define STEPS 5
#define D 3
#define M 500

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static double uni(void) {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return (double)(rng >> 11) / 9007199254740992.0;
}

static void die(int32_t st, const char* what) {
    char buf[512];
    abo_last_error(buf, sizeof buf);
    fprintf(stderr, "%s failed: status %d: %s\n", what, st, buf);
    exit(1);
}

int main(void) {
    static double X[(N0 + STEPS) * D], y[N0 + STEPS], Z[M * D], mu[M], var[M], mu_r[M], var_r[M];
    for (int i = 0; i < (N0 + STEPS) * D; ++i) X[i] = uni();
    for (int i = 0; i < N0 + STEPS; ++i) y[i] = sin(6.0 * X[i * D]) + X[i * D + 1] * X[i * D + 2];
    for (int i = 0; i < M * D; ++i) Z[i] = uni();
    abo_params p = {ABO_KERNEL_MATERN52, 0, 0.8, 1.3, 1e-3, 0.0, 0.0, 256, 0};
    abo_gp* g = NULL;
    int64_t info = 0;
    int32_t st, path = -1;
    if ((st = abo_create(&p, &g))) die(st, "abo_create");
    if ((st = abo_fit(g, X, N0, D, y, ABO_HOST, &info))) die(st, "abo_fit");
    for (int j = 1; j <= STEPS; ++j) {
        abo_gp* n = NULL;
        if ((st = abo_update(g, &p, NULL, X, N0 + j, D, y, ABO_HOST, &info, &path, &n))) die(st, "abo_update");
        if (path != ABO_UPDATE_APPENDED) { fprintf(stderr, "step %d: path %d, expected ABO_UPDATE_APPENDED\n", j, path); return 1; }
        abo_destroy(g);
        g = n;
    }
    abo_gp* r = NULL;
    if ((st = abo_create(&p, &r))) die(st, "abo_create");
    if ((st = abo_fit(r, X, N0 + STEPS, D, y, ABO_HOST, &info))) die(st, "abo_fit (refit)");
    if ((st = abo_predict(g, Z, M, D, ABO_HOST, mu, var, ABO_HOST))) die(st, "abo_predict");
    if ((st = abo_predict(r, Z, M, D, ABO_HOST, mu_r, var_r, ABO_HOST))) die(st, "abo_predict (refit)");
    double emu = 0.0, evar = 0.0;
    for (int i = 0; i < M; ++i) {
        if (fabs(mu[i] - mu_r[i]) > emu) emu = fabs(mu[i] - mu_r[i]);
        if (fabs(var[i] - var_r[i]) > evar) evar = fabs(var[i] - var_r[i]);
    }
    abo_gp* same = NULL;
    if ((st = abo_update(g, &p, NULL, X, N0 + STEPS, D, y, ABO_HOST, &info, &path, &same))) die(st, "abo_update (same data)");
    if (path != ABO_UPDATE_SHARED || same != g) { fprintf(stderr, "same data: path %d, expected ABO_UPDATE_SHARED\n", path); return 1; }
    abo_destroy(same);
    abo_destroy(g);
    abo_destroy(r);
    if (!(emu < 1e-9 && evar < 1e-9)) { fprintf(stderr, "appended vs refit: max|dmu| %.3e max|dvar| %.3e\n", emu, evar); return 1; }
    printf("c_update_harness ok: N=%d+%d d=%d max|dmu|=%.2e max|dvar|=%.2e\n", N0, STEPS, D, emu, evar);
    return 0;
}
