// Internal launcher interface between the C-ABI (api.hip) and the kernel translation units.
// Everything here is device-pointer based; no torch types, no host math.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace abo {

constexpr int TB = 128;  // block (tile) edge used by every blocked stage; all padded sizes are multiples of it
constexpr int MAX_P = 129; // outputs per point of a gradient-enhanced GP (f + d ≤ 128 partial derivatives; d ≤ 32: register-resident generator)

inline int64_t pad_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }

// ---- fp64 MFMA GEMM family (gemm.hip) -------------------------------------------------------
enum KMode { K_FULL = 0, K_A_LOWER = 1, K_A_UPPER = 2, K_B_LOWER = 3, K_B_UPPER = 4 };

struct GemmArgs {
    const double* A;      // [M][lda]   row-major, k contiguous
    const double* B;      // [N][ldb]   row-major, k contiguous  (C = A·Bᵀ)
    double* C;            // [M][ldc]
    double* Ct;           // optional transposed copy  Ct[j][i] = C[i][j]
    int64_t lda, ldb, ldc, ldct;
    int64_t sA, sB, sC, sCt;   // batch strides (elements)
    int M, N, K;          // M, N multiples of 128; K multiple of 16
    int kmode;            // K_FULL; K_A_LOWER: k < (ti+1)·128; K_A_UPPER: k ≥ ti·128; K_B_LOWER: k < (tj+1)·128 (B lower-triangular);
                          // K_B_UPPER: k ≥ tj·128 (B upper-triangular)
    int lower_only;       // 1: skip tiles with tj > ti (SYRK on the lower triangle)
    int batch;
    double alpha, beta;
    const int64_t* info;  // optional: if *info != 0 the kernel exits at once (failed factorisation)
    // split-k (batch == 1, beta == 0): the k range is cut into chunks of `ksplit` (multiple of 128), chunk z of a tile is computed by
    // its own workgroup into the partial product C + z·sC (a chunk outside the tile's triangular k range writes nothing);
    // launch_splitk_reduce sums the partials of every tile in chunk order (fixed order: deterministic).  For products with few output
    // tiles and a long k — the 128-row batches of the lockstep refinement against L⁻¹.
    int ksplit = 0;
    // split-k only: when 16 ≤ mrows ≤ 64 only the first mrows rows of A (a multiple of 16) matter and M == 128: the product is taken by
    // a kernel without LDS whose waves stream their 32 rows of B once and hold mrows/16 row groups of A — HBM-bound on B instead of
    // MFMA-bound on 128 rows (the lockstep refinement once most starts have finished)
    int mrows = 0;
    // square SYRK on the lower triangle (kmode K_FULL, batch 1), set by launch_gemm_nt: number of lower tiles T(T+1)/2 of a 1-D launch
    // whose workgroup → tile map is XCD-aware (gemm_nt_kernel); 0 = the plain 2-D launch
    int swz = 0;
    int swz_g = 4;        // tile rows per super-row of that map
};
hipError_t launch_gemm_nt(const GemmArgs& a, hipStream_t s);
// Which kernel and launch shape launch_gemm_nt gives a product (== ABO_GEMM_PATH_* of include/abo_hip.h): the one place the choice is
// made — pure host code, no GPU call; reads ABO_GEMM_SMALL (0 never / 1 always the small kernel) and ABO_GEMM_NO_SWIZZLE.
enum GemmPath {
    GEMM_PATH_INVALID = -2,    // split-k with batch != 1, beta != 0, a Ct or a ksplit that is no multiple of 128: launch_gemm_nt refuses it
    GEMM_PATH_NONE = -1,       // M, N or batch ≤ 0: nothing to do
    GEMM_PATH_TILED = 0,       // gemm_nt_kernel, 2-D grid of 128×128 tiles (× batch)
    GEMM_PATH_SWIZZLED = 1,    // gemm_nt_kernel, 1-D XCD-aware launch over the lower tiles of a square SYRK
    GEMM_PATH_SMALL = 2,       // gemm_nt_small_kernel: ≤ 64 tiles, K a multiple of 128, not in place
    GEMM_PATH_SKINNY = 3,      // split-k, gemm_skinny_kernel<mrows/16>
    GEMM_PATH_SPLITK = 4       // split-k, gemm_nt_kernel with one chunk per blockIdx.z
};
// tiles of the launch: Tm·Tn, or the tiles (ti, tj ≤ ti), tj < Tn under lower_only; × batch
inline int64_t gemm_nt_tiles(const GemmArgs& a) {
    const int64_t Tm = a.M / TB, Tn = a.N / TB;
    int64_t tiles = Tm * Tn;
    if (a.lower_only) {
        const int64_t q = Tm < Tn ? Tm : Tn;
        tiles = q * (q + 1) / 2 + (Tm - q) * Tn;
    }
    return tiles * a.batch;
}
int gemm_nt_path(const GemmArgs& a);
// The swizzled launch's workgroup → tile map in its two steps (gemm_nt_kernel documents the intent).
// Workgroup L of the padded 1-D grid of ⌈tiles/8⌉·8 → position Q in the tile sequence: XCD L & 7 takes the (L & 7)-th eighth; Q ≥ tiles: idle.
__host__ __device__ inline int gemm_swz_q(int L, int tiles) {
    const int per = (tiles + 7) >> 3;
    return (L & 7) * per + (L >> 3);
}
// Position Q < T(T+1)/2 → lower tile (ti, tj ≤ ti) of a T×T tile grid: the sequence runs through super-rows of G tile rows column by column
__host__ __device__ inline void gemm_swz_tile(int T, int G, int Q, int& ti, int& tj) {
    int g = (int)((sqrt(8.0 * (double)Q + 1.0) - 1.0) / (2.0 * G));        // super-row: G·g·(G·g+1)/2 tiles lie before it
    while ((G * (g + 1)) * (G * (g + 1) + 1) / 2 <= Q) ++g;
    while ((G * g) * (G * g + 1) / 2 > Q) --g;
    int w = Q - (G * g) * (G * g + 1) / 2;
    const int r0 = G * g;
    const int R = G < T - r0 ? G : T - r0;
    if (w < R * (r0 + 1)) {                                              // full columns 0 … r0: R tiles each
        tj = w / R;
        ti = r0 + w - tj * R;
    } else {                                                             // the triangle at the right end
        w -= R * (r0 + 1);
        int c = 1;
        while (w >= R - c) { w -= R - c; ++c; }
        tj = r0 + c;
        ti = tj + w;
    }
}
// out[r][c] = Σ_z P[z][r][c] over the chunks z that intersect the k range of column tile c/128 under `kmode` (K_FULL, K_B_LOWER,
// K_B_UPPER); P: nz partial products of rows × cols (leading dimension ldp, stride sP), K the full k length
hipError_t launch_splitk_reduce(const double* P, int64_t ldp, int64_t sP, int nz, int rows, int cols, int K, int ksplit, int kmode,
                                double* out, int64_t ldo, hipStream_t s);

// V = W·K_XZ restricted to k ≤ i (W lower-triangular), reduced on the fly to per-row-block column
// sums of squares: partial[ti][j] = Σ_{i in block ti} (Σ_k W[i][k]·Kxz[j][k])²
struct VarGemmArgs {
    const double* W;      // [Np][ldw]
    const double* Kxz;    // [Mc][ldk]   candidate-major chunk, k contiguous
    double* partial;      // [Np/128][ldp]
    int64_t ldw, ldk, ldp;
    int Np, Mc;           // multiples of 128
    int nvalid;           // rows ≥ nvalid (the view's N) are excluded from the norm
};
// variant 0: the 256-row kernel when Np is a multiple of 256, the 128-row kernel otherwise; 1: the 128-row kernel whatever Np (tests:
// the two agree bit for bit)
hipError_t launch_var_gemm(const VarGemmArgs& a, hipStream_t s, int variant = 0);

// ---- the same contraction on the int8 matrix pipe (ozaki.hip): exact products of fixed-point images of W and K_XZ through
// residues modulo n coprime moduli ≤ 256, Chinese-remainder reconstruction in fp64
constexpr int OZ_MAXMOD = 16;
struct OzPlan {
    int n;                       // number of moduli (8 … 16)
    int p[OZ_MAXMOD];            // 256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193
    double invp[OZ_MAXMOD];
    double c26[OZ_MAXMOD];       // 2^26 mod p (symmetric): the quantiser reduces x = xh·2^26 + xl as xh·c26 + xl
    double s1[OZ_MAXMOD], s2[OZ_MAXMOD];   // (P/p)·((P/p)⁻¹ mod p) split into a 41-bit head on a common grid and the rest
    double P1, P2, invP;         // P = Π p split the same way; 1/P
    int eP;                      // 2^eP ≤ P/4: the bound every exact integer dot product is kept under
};
bool oz_make_plan(int n, OzPlan* out);
size_t oz_w_bytes(int n, int Np);            // residue planes of W: n × pad256(Np)²
size_t oz_k_bytes(int n, int Np, int Mc);    // residue planes of a candidate chunk (and of its U): n × pad256(Mc) × pad256(Np)
int oz_k_scale(double kmax, int bits = 53);  // sK with rint(K·2^sK) ≤ 2^(bits−1) for 0 ≤ K ≤ kmax (bits = 53: the full-width image)
// W (lower-triangular, [Np][ldw]) → WR [n][Np256][Np256] int8, sexp[Np256] (row scales s_i), bad_row[Np256] (non-finite rows)
// rows ≥ nvalid (identity padding, or the remains of a discarded appended branch) become zero planes
hipError_t oz_prepare_w(const OzPlan& pl, const double* W, int64_t ldw, int Np, int nvalid, int8_t* WR, int* sexp, int* bad_row, hipStream_t s,
                        int kper = 1, int ktg = 0);
// ---- the short plan of the pruned selection's bound pass (ozaki.hip: "the guarded bound") ----
// K bits of a short plan with exponent budget eP over `rows` factor rows: K' ≤ 2^(bK−1), W' keeps bW = eP − bK bits below its row's L1 norm
int oz_bound_kbits(int eP, int rows);
// The first `rows` (a multiple of 256, ≤ pad256(Np)) rows of W under the short plan `pl`: WRb [pl.n][rows][pad256(Np)] int8 (the row
// stride of the full planes, so that the residue GEMM walks both with one stride; only the k < rows bytes of a row are written or
// read), sexp_b / bad_row_b / delta [rows]: delta[i] ≥ |Ṽ_ij − v_ij| + the roundings of either side, for Ṽ the short plan's
// reconstruction at (sexp_b[i], sK_b) and v the reconstruction of the plan `full` at its own row scale and sK_full.
hipError_t oz_prepare_w_bound(const OzPlan& pl, const OzPlan& full, const double* W, int64_t ldw, int Np, int nvalid, int rows, int kbits, int sK_b,
                              int sK_full, double kmax, int8_t* WRb, int* sexp_b, int* bad_row_b, double* delta, hipStream_t s);
constexpr int OZ_CTR_INTS = 16;
struct OzVarArgs {
    const OzPlan* plan;
    const double* Kxz;     // [Mc][ldk] candidate-major chunk (fp64, as launch_var_gemm takes it)
    int64_t ldk;
    const int8_t* WR; const int* sexp; const int* bad_row;
    int8_t* KR;            // scratch: oz_k_bytes
    int8_t* U;             // scratch: oz_k_bytes
    int* bad_col;          // scratch: pad256(Mc) + OZ_CTR_INTS ints (the persistent GEMM's tile counters sit behind the flags)
    double* partial;       // [Np/128][ldp]
    int64_t ldp;
    int Np, Mc, nvalid, sK;
    int kper = 1, ktg = 0; // gradient-enhanced model: training rows k with k % kper != 0 are scaled by 2^−ktg in the chunk's image
    int planes_ready = 0;  // 1: KR / bad_col were written by the generator (KgenArgs::res), skip the quantisation pass
    // all outputs of a gradient-enhanced model's candidates: chunk row r is output (r0 + r) % rper of its point (rmode 1, point-major
    // rows) or output (r0 + r) / rpts (rmode 2, rows by outputs); derivative rows (output != 0) are scaled by 2^-ktg in the chunk's
    // image as well, and their column sums by 2^(2 ktg) on the way out.  rmode 0: every row is a function value.
    int rmode = 0, rper = 1;
    int64_t r0 = 0, rpts = 1;
    // > 0: only the first rblocks 256-row blocks of W are contracted — partial[tb] for tb < 2·rblocks, the sum of squares over the
    // first min(nvalid, 256·rblocks) rows of V, bit for bit what the full call writes there (the buffers keep their full layout)
    int rblocks = 0;
    // the guarded bound (rblocks > 0 only): delta[i] per contracted row — the column sums are of max(|V_ij| − delta[i], 0)²; nullptr =
    // the exact sums.  w_plane: bytes between the residue planes of WR when they are not the full pad256(Np)² planes (0 = they are)
    const double* delta = nullptr;
    int64_t w_plane = 0;
    double* Vout = nullptr;     // when given: V = W.K_XZ itself, [Mc][ldv] fp64 (candidate-major), instead of the column sums of squares
    int64_t ldv = 0;
    hipEvent_t ev_quant = nullptr, ev_gemm = nullptr;   // optional: recorded after the quantisation / after the GEMM
    // optional, HOST: where the owner remembers which tile-counter block is known to hold zeros.  The reconstruction kernel that ends a
    // call zeroes the counters again, so the next call on the same scratch needs no memset in front of its GEMM; the slot is cleared
    // while a call is between its GEMM and its reconstruction (an error in there leaves the counters dirty: the next call memsets).
    int** ctr_clean = nullptr;
};
hipError_t launch_var_ozaki(const OzVarArgs& a, hipStream_t s);

// ---- the stages of launch_var_ozaki / oz_prepare_w / oz_prepare_w_bound, one launcher each, on raw pointers (ozaki.hip).  Each returns
// hipErrorInvalidValue, and launches nothing, for arguments its kernel cannot take.
constexpr int OZ_SEXP_MAX = 960;            // no row scale above this (oz_row_scale: the clamp)
constexpr int OZ_SEXP_BAD = -(1 << 20);     // the row scale of a row whose norm is not finite or ≥ 1e300: flagged by the quantiser, NaN in V
// the guard of a short plan (ozaki.hip: "the guarded bound"); delta == nullptr: none
struct OzGuardArgs {
    double* delta;          // [Np256] or nullptr: no guard (every plan but the short one)
    int eP_full, sK_b, sK_full;
    double kmax, rec_b, rec_full;
};
// oz_rowscale_kernel: sexp[0 .. rows256) (and gd.delta) from the first nrows rows of the lower-triangular W; rows ≥ nrows get 0
hipError_t launch_oz_rowscale(const double* W, int64_t ldw, int nrows, int rows256, int eP, int* sexp, int kper, int ktg, int kbits,
                              const OzGuardArgs& gd, hipStream_t s);
// oz_quant_kernel: fp64 → n residue planes in the device layout (abo_oz_dev.h: oz_plane_off)
struct OzQuantArgs {
    const double* in;
    int64_t ldin;
    int rows_in, cols_in, rows_out, cols_out;
    int lower;                 // 1: entries with k > r are zero (W = L⁻¹; the stored zeros are not even read)
    const int* srow;
    int sconst;
    int kper, ktg;             // columns k with k % kper != 0 get 2^ktg on top (kper ≤ 1: none)
    int rmode, rper, rtg;      // rows whose output index (oz_row_output) is not 0 get 2^rtg on top (rmode 0: none)
    int64_t r0, rpts;
    int8_t* out;
    int64_t ld, plane;
    int* bad;                  // [rows_out] or nullptr
    OzPlan pl;
};
hipError_t launch_oz_quant(const OzQuantArgs& q, hipStream_t s);
// 256-row blocks of W the residue GEMM, U and the reconstruction cover: all Np256 / 256 of them, or the first rblocks (OzVarArgs::rblocks)
inline int oz_gemm_row_blocks(int Np256, int rblocks) { return rblocks > 0 && rblocks < Np256 / 256 ? rblocks : Np256 / 256; }
// the persistent residue GEMM: U (oz_u_block layout, row blocks as above × Mc256 / 256 column blocks × pl.n moduli) from the planes
// KR [n][Mc256][Np256] and WR [n][·][Np256] (plane stride w_plane bytes, 0 = Np256²; LOWER-TRIANGULAR: the kernel skips the units of
// a diagonal block that lie above the diagonal).  ctr: 8 tile counters, zero on entry; the kernel leaves them advanced.
hipError_t launch_oz_gemm(const OzPlan& pl, const int8_t* KR, const int8_t* WR, int8_t* U, int Np256, int Mc256, int rblocks, int64_t w_plane,
                          int* ctr, hipStream_t s);
// the tile list of that launch as the kernel decodes it (host): tiles[8·per_list] = the decoded ticket of every (list y, q < per_list),
// y-major — ti | tj << 9 | l << 20, or −1 for a padding block; returns 8·per_list, the launcher's `blocks` (tiles may be null)
int64_t oz_gemm_tickets(int Ti, int Tj, int n, int32_t* tiles);
// the reconstruction: V itself (V != nullptr: oz_crt_v_kernel), or the column sums of squares per 128-row block (oz_crt_kernel: exact,
// or guarded when delta is given; the compile-time moduli count where there is one, unless generic is set)
struct OzCrtLaunch {
    const OzPlan* plan;
    const int8_t* U; int Ti;
    const int* sexp; int sK;
    const int* bad_row; const int* bad_col;
    int Np, Mc, nvalid;
    int rmode, rper, rtg; int64_t r0, rpts;
    int* ctr_reset;            // the GEMM's counters, zeroed by the kernel (or nullptr)
    const double* delta;       // the guard (sums only)
    double* partial; int64_t ldp;
    double* V; int64_t ldv;
    int generic;               // 1: the run-time moduli loop (NM = 0) also at 14 and 8 moduli
};
hipError_t launch_oz_crt(const OzCrtLaunch& c, hipStream_t s);

// ---- kernel-matrix generation (kgen.hip) ----------------------------------------------------
struct KgenArgs {
    const double* Xs;     // [Np][dp]   training points, pre-scaled by 1/ell, zero padded
    const double* Z;      // [M][d]     raw candidate points (caller layout), scaled on load
    const double* alpha;  // [Np] zero padded, or nullptr (no mean)
    double* Kout;         // [Mc][ldk]  Kout[j][k] = sigma_f2·kappa(||Xs_k − s·z_j||²), 0 for k ≥ N
    double* mu;           // [Mc] mean_c + Σ_k Kout[j][k]·alpha[k], or nullptr
    int64_t ldk;
    int64_t M;            // number of valid candidates overall
    int64_t j0;           // first candidate of this chunk
    int Mc;               // padded chunk rows (multiple of 16)
    int N, Np, d, dp, family;
    double s, sigma_f2, mean_c;
    // gradient-enhanced GP (pt > 1): training rows are (output q', point i) by outputs, pt = d+1 outputs per
    // point, Np pads pt·N; candidate rows carry pc outputs each (1 = function value only, pt = all outputs)
    int pt = 1, pc = 1, point_major = 0;
    int dlogell = 0;      // gradient-enhanced GP only: write dK/dlog(ell) instead of K (hyper-parameter gradient)
    int rvalid = 0;       // gradient-enhanced GP only: valid training rows when not N·pt (a partly appended point)
    double mean_vec[MAX_P] = {0};   // prior mean per output (gradConstMean)
    // int8-residue engine: write the residue planes of the kernel values in the same pass (StandardGP, dp ≤ 32):
    // res[l][j][k] = sym_residue(rint(K[j][k]·2^res_sK), p_l), res_bad[j] = 1 for a candidate with a non-finite kernel value
    // (zeroed by the launcher); Kout may then be nullptr
    int8_t* res = nullptr;
    int64_t res_ld = 0, res_plane = 0;
    int* res_bad = nullptr;
    int res_n = 0, res_sK = 0;
    int res_ktg = 0;      // gradient-enhanced GP: derivative training rows and derivative candidate outputs each carry 2^-res_ktg on top
    int res_kmax = 0;     // StandardGP: > 0 (a multiple of 128) = the launch covers the training columns k < res_kmax alone (the rest is
                          // never read by a contraction limited to the first res_kmax rows of the triangular W): planes for them, and
                          // mu = mean_c + their part of the sum — the other columns' part comes from launch_kgen_tail; 0 = all columns
};
// true when launch_kgen honours KgenArgs::res for this shape and n moduli (the fused output is instantiated for the default plan, and
// for the short plans of the pruned selection's bound pass — 8, 9, 10 moduli — in the partial launch res_kmax > 0 of a StandardGP alone)
inline bool kgen_short_moduli(int n) { return n >= 8 && n <= 10; }
inline bool kgen_writes_residues(const KgenArgs& a, int n) {
    return a.dp <= 32 && !a.dlogell && (n == 14 || (kgen_short_moduli(n) && a.res_kmax > 0 && a.pt == 1));
}
hipError_t launch_kgen(const KgenArgs& a, hipStream_t s);
// ---- value-only model against (f, ∇f) query outputs (kgen_deriv.hip; abo_predict_deriv) ----
// For the chunk's points j < npts (global index pt0 + j) and p = d + 1, with e = (Xs_k − s·z_j), u = ‖e‖²:
//   Kout[j·p][k] = sigma_f2·φ(u),   Kout[j·p + c + 1][k] = −sigma_f2·φ'(u)·2e_c·s   for k < N, 0 for N ≤ k < Np
//   mu_rows[j·p + q] = (q == 0 ? mean_c : 0) + Σ_k Kout[j·p + q][k]·alpha[k]   (a fixed order: the same bits on every launch)
// Rows npts·p ≤ r < rows_pad of Kout (columns < Np) and of mu_rows are written as 0; nothing else is.  Families SE, Matérn-5/2 and
// Matérn-7/2 (φ, φ' of kgen_grad_core.h), d ≤ 32 with dp ∈ {1, 2, 4, 8, 16, 32}; hipErrorInvalidValue, and no launch, for anything else,
// for a chunk that leaves [0, M) and for rows_pad < npts·p.
struct KgenDerivArgs {
    const double* Xs;     // [Np][dp]   training points, pre-scaled by 1/ell, zero padded
    const double* Z;      // [M][d]     raw query points, scaled on load
    const double* alpha;  // [Np] (only k < N is read), or nullptr: zeros
    double* Kout;         // [rows_pad][ldk]
    double* mu_rows;      // [rows_pad], or nullptr
    int64_t ldk;
    int64_t M, pt0;       // query points overall; first point of this chunk
    int npts;             // points of this chunk
    int64_t rows_pad;     // rows of Kout the launch writes (≥ npts·(d + 1): what the contraction behind it reads)
    int N, Np, d, dp, family;
    double s, sigma_f2, mean_c;
};
hipError_t launch_kgen_deriv(const KgenDerivArgs& a, hipStream_t s);
// ---- the μ-only tail of the pruned selection's bound pass (kgen_tail.hip) ----
// over the N training points: norms[0] = Σ_{k ≥ k0} |alpha_k|, norms[1] = Σ_k |alpha_k|, norms[2] = max_{k ≥ k0} |Xs_k|² — one
// workgroup, fixed order
hipError_t launch_tail_norms(const double* Xs, const double* alpha, int N, int dp, int k0, double* norms, hipStream_t s);
// For the chunk's candidates j (global index gj = j0 + j < M):
//   mu_tail[gj] = sigma_f2·Σ_{k0 ≤ k < N} alpha_k·κ̃(r²_jk), κ̃ = kappa_tail of the EXPANDED squared distance |x|² + |z|² − 2x·z
//   eps[gj]     ≥ |(head + mu_tail) − μ| for the μ of a full launch_kgen and the head of one limited to res_kmax = k0
// (derivation: kgen_tail.hip).  A candidate with a non-finite coordinate, or |x|² + |z|² ≥ TAIL_W_MAX, gets mu_tail = NaN.
struct KgenTailArgs {
    const double* Xs;     // [Np][dp]  only the rows k < N are read
    const double* Z;      // [M][d]
    const double* alpha;  // [Np]      only the entries k < N are read
    const double* norms;  // [3], launch_tail_norms with the same k0
    double* mu_tail;      // [M]
    double* eps;          // [M]
    int64_t M, j0;
    int Mc;               // padded chunk rows (multiple of 16)
    int N, Np, k0, d, dp, family;
    double s, sigma_f2, mean_c;
    const float* Xf = nullptr;   // launch_kgen_tail32 alone: the rows k ≥ k0 of Xs in fp32, pair-interleaved (launch_tail32_stage with the same k0); null: rounded in the kernel
};
hipError_t launch_kgen_tail(const KgenTailArgs& a, hipStream_t s);
// test hook: out[i] = kappa_tail(family, d2[i]) (abo_kappa.h)
hipError_t launch_kappa_tail_test(int family, const double* d2, double* out, int64_t n, hipStream_t s);
// ---- the head of the M-wide first bound level in one fused kernel (kgen_head32.hip) ----
// For every candidate gj < M, over the first R = 256·rblocks training points / rows of W (R ≤ N):
//   head[gj] = mean_c + sigma_f2·Σ_{k<R} alpha_k·κ(r²_jk)   in fp64, the generator's arithmetic per pair
//   ssq[gj]  ≤ the full pass's computed Σ_i v_ij² (V = W·K_XZ): (1 − c)·Σ_{i<R} max(|Ṽ_ij| − delta[i], 0)², Ṽ = fl32(W)·fl32(K) on the fp32
//              matrix pipe; NaN for a candidate with a non-finite kernel value
// A preparation launch in front writes Wf (R·R floats, fragment order), l1[i] = ‖W_i‖₁ and delta[i] ≥ |Ṽ_ij − v_ij| (+Inf: a flagged
// row, which contributes 0).  eP_full / sK_full / rec_full: the full pass's residue plan (its exponent budget, the scale of its image of
// K and its reconstruction error in integer units), which delta covers.  Nothing behind M or R is written.
struct KgenHead32Args {
    const double* Xs;     // [Np][dp]  only the rows k < R are read
    const double* Z;      // [M][d]
    const double* alpha;  // [Np]      only the entries k < R are read
    const double* W;      // [Np][ldw] only the rows i < R, columns k ≤ i
    int64_t ldw;
    float* Wf;            // scratch [R·R]
    double* delta;        // [R]
    double* l1;           // [R]
    double* head;         // [M]
    double* ssq;          // [M]
    int64_t M;
    int N, Np, R, d, dp, family;
    double s, sigma_f2, mean_c;
    int eP_full, sK_full;
    double rec_full;
};
hipError_t launch_kgen_head32(const KgenHead32Args& a, hipStream_t s);
// NLML gradient reduction: Σ_ij (Kinv − ααᵀ)_ij ∂K_ij/∂log ℓ over the lower tiles, plus tr(Kinv), αᵀα, αᵀδ
struct NlmlGradArgs {
    const double* Xs;      // [Np][dp]
    const double* Kinv;    // [Np][ld]  lower 128-tiles valid
    const double* alpha;   // [Np]
    const double* delta;   // [Np]
    double* partial;       // [Np/16]
    double* out;           // [4]
    int64_t ld;
    int N, Np, dp, family;
    double sigma_f2;
};
hipError_t launch_nlml_grad(const NlmlGradArgs& a, hipStream_t s);
// one length scale per coordinate (dp ≤ 32), the same sweep: a.partial is [Np/16][dp] here and
// out_ard[c] = Σ_ij (Kinv − ααᵀ)_ij ∂K_ij/∂log ℓ_c for c < dp (exactly 0 for the padded c ≥ d); a.out[1..3] as above, a.out[0] = 0
hipError_t launch_nlml_grad_ard(const NlmlGradArgs& a, double* out_ard, hipStream_t s);
// same reductions with dK/dlog(ell) given as a matrix D (gradient-enhanced GP: D comes from kgen with dlogell = 1):
// out[0] = sum_{i,k<N} (Kinv[i][k] - alpha_i alpha_k) D[i][k]  (lower 128-tiles, strictly-lower ones counted twice), out[1..3] as above
hipError_t launch_nlml_grad_matrix(const NlmlGradArgs& a, const double* D, int64_t ldd, hipStream_t s);
// D[i][k] = sigma_f2·∂kappa/∂log ℓ(‖Xs_i − Xs_k‖²) for i, k < N, 0 elsewhere: the full symmetric Np × Np matrix (leading dimension ldd)
// of an ordinary model (the dlogell path of launch_kgen is the gradient-enhanced one); closed forms q(d2)·d2, finite at d2 = 0
hipError_t launch_dkdlogell(const double* Xs, int N, int Np, int dp, int family, double sigma_f2, double* D, int64_t ldd, hipStream_t s);

// ---- leave-one-out cross-validation (loo.hip) -------------------------------------------------
struct LooArgs {
    const double* WT;      // [≥ N][ld] upper-triangular: row i holds column i of W = L⁻¹
    const double* alpha;   // [≥ N]
    const double* delta;   // [≥ N]  y − mean_c
    double* mu;            // [N] or nullptr   y_i − alpha_i/B_ii,  B_ii = Σ_{i ≤ k < N} WT[i][k]²
    double* var;           // [N] or nullptr   1/B_ii
    double* lpd;           // [N] or nullptr   −½ log var − (y − mu)²/(2 var) − ½ log 2π
    double* partial;       // [loo_diag_blocks(N)]
    double* nlpl;          // [1]  −Σ_i lpd[i], fixed order
    int64_t ld;
    int N;
    double mean_c;
};
int loo_diag_blocks(int N);
hipError_t launch_loo_diag(const LooArgs& a, hipStream_t s);
// B[i][j] = B[j][i] on the 128-tiles above the diagonal of the Np × Np matrix B (lower tiles valid on the way in)
hipError_t launch_loo_mirror(double* B, int64_t ld, int Np, hipStream_t s);
// out[0..3) = ∂nlpl/∂(log ℓ, log sigma_f2, log noise) from the rows of T = B·∂K/∂log ℓ and B = K̃⁻¹ (both complete, [Np][ld])
struct LooGradArgs {
    const double* T;
    const double* B;
    const double* alpha;   // [Np]
    double* partial;       // [3·loo_grad_blocks(N)]
    double* out;           // [3]
    int64_t ld;
    int N;
    double noise;          // the noise the factor was built with
};
int loo_grad_blocks(int N);
hipError_t launch_loo_grad_rows(const LooGradArgs& a, hipStream_t s);

// ---- joint posterior covariance between point sets (cov.hip) ----------------------------------
// C[i][j] = sigma_f2·kappa(‖As_i − Bs_j‖²) for i < Ma, j < Mb and 0 in the padding of the pad128(Ma) × pad128(Mb) block C (leading
// dimension ldc); As / Bs: the points scaled by 1/ell, zero padded to [pad128(M)][dp] (launch_scale_points).  Differences formed
// directly and summed in coordinate order: As == Bs gives a block that is symmetric bit for bit with exactly sigma_f2 on its
// diagonal.  sym = 1 (As == Bs): only the 128-tiles with tj ≤ ti are written.
hipError_t launch_cov_prior(const double* As, const double* Bs, int Ma, int Mb, int dp, int family, double sigma_f2, int sym, double* C,
                            int64_t ldc, hipStream_t s);
// out[i·Mb + j] = C[i][j] for i < Ma, j < Mb; sym = 1: + 1e-18 on the diagonal (abo_predict's latent-variance jitter)
hipError_t launch_cov_pack(const double* C, int64_t ldc, int Ma, int Mb, int sym, double* out, hipStream_t s);

// ---- knowledge gradient over a discrete decision set (kg.hip; abo_acq_kg) ----------------------
// Row i's lines: intercept asign·a[j], slope B[i·ldb + j]/den[i] for j < Mb (den null: the slopes as they are), and — self_b given — the
// row's own line (asign·self_a[i], self_b[i]).  val[i] = E[max_j (a_j + b_ij·Z)] − max_j a_j exactly (sort by (b, a), upper-envelope scan,
// Σ Δb·h(−|c|) in envelope order); nenv[i] (may be null) = lines on the envelope.  den[i] == 0: val 0.0, nenv 1; a non-finite intercept or
// slope in the row: val NaN, nenv 0.  One workgroup per row, the lines in LDS: kg_lds_bytes(Mb) of it, Mb ≤ KG_MAX_LINES.
constexpr int KG_MAX_LINES = 8192;
struct KgArgs {
    const double* a; const double* B; int64_t ldb;
    const double* den; const double* self_a; const double* self_b;
    double asign;
    int Ma, Mb;
    int P;                 // set by the launcher: the power of two ≥ Mb
    double* val; int* nenv;
};
inline int kg_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
size_t kg_lds_bytes(int Mb);
hipError_t launch_kg_rows(KgArgs a, hipStream_t s);
// per candidate i < Ma: v_i = C[i][i] (C given: the symmetric form's diagonal) or sigma_f2 − Σ_{k<R} V[i][k]² (one wave per row, a fixed
// order), + 1e-18; den[i] = sqrt(v_i + noise), 0 where v_i + noise ≤ 1e-12; self_b[i] = v_i/den[i] (0 with den)
hipError_t launch_kg_prep(const double* V, int64_t ldv, int R, const double* C, int64_t ldc, int Ma, double sigma_f2, double noise,
                          double* den, double* self_b, hipStream_t s);
// test hook: out[i] = kappa(family, d2[i]) with the device math the generator uses
hipError_t launch_kappa_test(int family, const double* d2, double* out, int64_t n, hipStream_t s);
// K[i][i] += noise for i < N; K[i][i] = 1 for N ≤ i < Np (identity padding keeps the factor PD)
hipError_t launch_diag_fix(double* K, int64_t ld, int N, int Np, double noise, hipStream_t s, int64_t* info_reset = nullptr);
// A[i][i] = v for lo ≤ i < hi
hipError_t launch_set_diag(double* A, int64_t ld, int lo, int hi, double v, hipStream_t s);
// Xs[i][c] = X[i][c]·s (zero padded to [Np][dp])
hipError_t launch_scale_points(const double* X, double* Xs, int N, int Np, int d, int dp, double s, hipStream_t st);
// a bordered append's new observation (x on the HOST, d ≤ APPEND_POINT_MAXD) → rows of Xraw / Xs, y, δ = y − m, *info = 0: one launch
constexpr int APPEND_POINT_MAXD = 64;
hipError_t launch_append_point(const double* x_host, int d, int dp, double s, double y, double mean_c, double* Xraw_row, double* Xs_row,
                               double* y_at, double* delta_at, int64_t* info, hipStream_t st);
// everything in front of a fit's kernel matrix in one launch: the model's copies of the caller's X / y (when Xsrc / ysrc are not
// those copies already), scaled zero-padded points, centred targets, alpha = 0
hipError_t launch_fit_prep(const double* Xsrc, const double* ysrc, double* Xraw, double* ybuf, double* Xs, double* delta, double* alpha,
                           int N, int Np, int d, int dp, double s, double mean_c, hipStream_t st);

// ---- factorisation pieces (chol.hip) --------------------------------------------------------
// factor the 128×128 diagonal block at (r0,r0) of K in place (lower), write its inverse into the
// matching diagonal block of W (lower) and WT (upper = transposed); on a non-positive pivot set
// *info = r0 + j + 1 (if still 0) and leave.
hipError_t launch_chol_diag(double* K, double* W, double* WT, int64_t ld, int r0, int64_t* info, hipStream_t s);
// The whole fit of an N ≤ 128, d ≤ 16 model in ONE launch of the diagonal-block kernel (mode 3): writes Xs [128][dp], delta,
// L (→ K), L⁻¹ (→ W, WT), alpha, scal = {log det, δᵀα}; K / W / WT have leading dimension 128.  *info as launch_chol_diag.
struct FitSmallArgs {
    const double* Xraw;   // [N][d] raw inputs (device): the model's copy, or the caller's array when Xkeep is set
    const double* y;      // [N]
    double* Xkeep;        // non-null: the kernel also writes the model's own copies of the inputs it read (the caller's device
    double* ykeep;        //           arrays go straight into the one launch: no staging copies in front of it)
    double* Xs;           // [128][dp]
    double* delta;        // [128]
    double* alpha;        // [128]
    double* scal;         // [2]
    int N, d, dp, family;
    double s, sigma_f2, noise, mean_c;
};
hipError_t launch_fit_small(double* K, double* W, double* WT, int64_t* info, const FitSmallArgs& fs, hipStream_t s);
// the same split for the panel chain: potf2 (factor + the eight 16×16 diagonal sub-block inverses, which go to their final
// places in W / WT), the panel solve below the block as a blocked triangular solve on L (rows r0+128 … r0+128+nrows), and —
// once, after the factorisation — the 128×128 inverses of ALL diagonal blocks in one batched launch
hipError_t launch_potf2_diag(double* K, double* W, double* WT, int64_t ld, int r0, int64_t* info, hipStream_t s, double* P, bool zero_rows = false);
constexpr size_t TRSM_STREAM_BYTES = 144 * 64 * sizeof(double);      // the packed operands potf2_pipe_kernel leaves for trsm_stream_kernel
hipError_t launch_trsm_stream(double* K, const double* P, int64_t ld, int r0, int nrows, const int64_t* info, hipStream_t s);
hipError_t launch_trtri_diag_batched(double* K, double* W, double* WT, int64_t ld, int nblocks, int64_t* info, hipStream_t s);
// out[i] = Σ_{k ≤ i} Wm[i][k]·v[k]   (lower == 1)   or   Σ_{k ≥ i} Wm[i][k]·v[k]   (lower == 0)
hipError_t launch_trmv(const double* Wm, int64_t ld, const double* v, double* out, int Np, int lower, hipStream_t s);
// out[0] = 2·Σ_{i<N} log L[i][i];  out[1] = Σ_{i<N} delta[i]·alpha[i]
hipError_t launch_nlml_terms(const double* L, int64_t ld, const double* delta, const double* alpha, int N, double* out, hipStream_t s);
// delta[i] = y[i] − c (i < N), 0 for padding
hipError_t launch_center(const double* y, double* delta, int N, int Np, double c, hipStream_t s);
// gradient-enhanced GP: targets arrive by outputs (y_abi[q·N + i], prep_output of the reference) and are kept point-major
// (ybuf[i·p + q]); delta[r] = ybuf[r] − mean[r % p] for r < N·p, 0 up to Np
struct MeanVec { double c[MAX_P]; };
hipError_t launch_center_grad(const double* y_abi, double* ybuf, double* delta, int N, int p, int Np, MeanVec mean, int y_point_major,
                              hipStream_t s);

// bordered append (chol.hip): given k = k(X,x*), l = W·k, v = Wᵀ·l, write row N of L and W, column N of WT,
// the new alpha and the down-date vector vext = [−v ; 1]; scal = {l_nn², β, l_nn, kᵀα}; *info = N+1 if l_nn² ≤ 0
struct AppendArgs {
    double* L; double* W; double* WT;
    int64_t ld;
    const double* krow; const double* lvec; const double* vvec;
    const double* alpha_old; double* alpha_new; double* vext;
    const double* delta;
    int N, cap;
    double kss;              // k(x*,x*) + noise
    double* scal;
    int64_t* info;
};
hipError_t launch_append(const AppendArgs& a, hipStream_t s);

// ---- blocked bordered append (append_batch.hip): k ≤ APPEND_BATCH_MAX new points in one step, kp = k padded to 16 ----------------
constexpr int APPEND_BATCH_MAX = 64;
// rows of Xraw / Xs / ybuf / delta for the k new points Xb [k][d], yb [k] (device); *info = 0
hipError_t launch_append_batch_points(const double* Xb, const double* yb, int k, int d, int dp, double s, double mean_c, double* Xraw_rows,
                                      double* Xs_rows, double* y_at, double* delta_at, int64_t* info, hipStream_t st);
// Kb [N + k][kp]: rows j < N = k(x_j, new point i), rows N + jj = the new points among themselves (bitwise symmetric, σ_f² on the
// diagonal), zero in columns ≥ k.  Xs_new [k][dp] scaled, Xraw [N + k][d]; launch_cand_newcol's arithmetic.
hipError_t launch_append_batch_newcols(const double* Xs_new, const double* Xraw, double* Kb, int N, int k, int d, int dp, int family,
                                       double s, double sigma_f2, hipStream_t st);
// out [N][kp] = tri(Wm)·V on the fp64 matrix pipe, V [N][kp]; lower as launch_trmv; only rows and columns < N of Wm are used.
// part: tri_skinny_part_doubles(N, kp) doubles of scratch.  kp a multiple of 16 up to 64, ld a multiple of 4 and ≥ N padded to 16.
size_t tri_skinny_part_doubles(int N, int kp);
hipError_t launch_tri_skinny(const double* Wm, int64_t ld, const double* V, double* out, double* part, int N, int kp, int lower,
                             hipStream_t s);
// BᵀB and K_bᵀα in append_batch_gram_blocks(N) ordered partial sums (gpart: that many × (kp² + kp) doubles), then the k × k part in one
// workgroup: sm = {L_s [kp][kp], L_s⁻¹ [kp][kp], β [kp]}, scal = {2·Σ log diag L_s, ‖L_s⁻¹r‖²}; a non-positive pivot j sets
// *info = N + j + 1 (if it was 0) and writes nothing else.  Kb as launch_append_batch_newcols leaves it, delta_b: the k centred targets.
int append_batch_gram_blocks(int N);
hipError_t launch_append_batch_small(const double* Bm, const double* Kb, const double* alpha, const double* delta_b, int N, int k,
                                     double noise, double* gpart, double* sm, double* scal, int64_t* info, hipStream_t s);
// rows N … N+k−1 of L and W, the matching columns of WT, α' (zero from N + k to cap); nothing when *info ≠ 0
struct AppendBatchArgs {
    double* L; double* W; double* WT;
    int64_t ld;
    const double* B; const double* C;        // [N][kp]: W·K_b and Wᵀ·B
    const double* sm;                        // launch_append_batch_small's
    const double* alpha_old; double* alpha_new;
    int64_t N, cap;
    int k, kp;
    const int64_t* info;
};
hipError_t launch_append_batch_write(const AppendBatchArgs& a, hipStream_t s);

// ---- posterior epilogue + selection (misc.hip) ----------------------------------------------
struct FinalizeArgs {
    const double* partial;   // [T][ldp]
    const double* mu_in;     // [Mc]
    double* mu_out;          // [M] or nullptr (global arrays, indexed j0 + j)
    double* var_out;         // [M] or nullptr
    double* score_out;       // [M] or nullptr
    int64_t ldp, j0, M;
    int T, Mc;
    int kind;                // ABO_ACQ_*, or −1 for none
    double sigma_f2, p0, best_y;
    // gradient-enhanced GP: rows carry pc outputs of Mpts points; prior variance of a gradient output
    double prior_grad = 0.0;
    int pc = 1, point_major = 0;
    int64_t Mpts = 0;
    // bound pass of the pruned selection: mu_in holds the head of the mean; mu_tail [M] (global index) its tail on the way in and
    // μ̃ = head + tail on the way out, mu_eps [M] the proven |μ̃ − μ| — var / score are taken at μ̃ − ε
    double* mu_tail = nullptr;
    const double* mu_eps = nullptr;
    // … with the fused first-level head (kgen_head32.hip): the head of the mean and the guarded sum of squares by GLOBAL index, in
    // place of mu_in and of the row blocks of partial
    const double* head_g = nullptr;
    const double* ssq_g = nullptr;
};
hipError_t launch_finalize(const FinalizeArgs& a, hipStream_t s);

// gradient-enhanced GP: per-point p×p posterior covariance (+ mean, + GradientNormUCB score) from V = L⁻¹K_XZ
struct GradCovArgs {
    const double* V;          // [points·p][ldv], point-major rows
    const double* mu_rows;    // [points·p]
    int64_t ldv;
    int R, p;
    int64_t pt0;              // global index of the chunk's first point
    double prior0, prior_g, beta;
    double* cov_out;          // [M][p][p] or nullptr
    double* mu_out;           // [M][p] or nullptr
    double* score_out;        // [M] or nullptr
};
hipError_t launch_grad_cov(const GradCovArgs& a, int npoints, hipStream_t s);

// resident-candidate kernels (C5)
// mu[j] += c[j]·beta ; var[j] −= c[j]²/s2        (posterior down-date after a bordered append)
hipError_t launch_downdate(double* mu, double* var, const double* c, int64_t M, double beta, double s2, hipStream_t s);
// resident K_ZX (candidate-major, ld doubles per candidate) of a candidate set:
//   newcol: Kzx[j][col] = sigma_f2·kappa(‖s·z_j − Xs[col]‖²) for all M candidates (the column of a just-appended point)
//   gemv:   c[j] = Σ_{k<n} Kzx[j][k]·v[k]   (the O(N·M) down-date as one streaming pass, no kernel evaluations)
hipError_t launch_cand_newcol(const double* Xs, const double* Z, double* Kzx, int64_t ld, int64_t M, int col, int d, int dp,
                              int family, double s, double sigma_f2, hipStream_t st);
// gradient-enhanced model: column `col` = training row (point pt, output q) against the function value of every candidate
hipError_t launch_cand_newcol_grad(const double* Xs, const double* Z, double* Kzx, int64_t ld, int64_t M, int col, int pt, int q,
                                   int d, int dp, int family, double s, double sigma_f2, hipStream_t st);
hipError_t launch_cand_gemv(const double* Kzx, int64_t ld, const double* v, int n, int64_t M, double* c, hipStream_t s);
// score[j] = acq(mu[j], var[j])
hipError_t launch_score(const double* mu, const double* var, double* score, int64_t M, int kind, double p0, double best_y,
                        hipStream_t s);
// f[j], dmu[j], dvar[j] = the epilogue's value and its partial derivatives with respect to μ and σ² (what the refinement evaluates)
hipError_t launch_score_partials(const double* mu, const double* var, double* f, double* dmu, double* dvar, int64_t M, int kind, double p0,
                                 double best_y, hipStream_t s);

// rec = {tv[0], (double)ti[0], mu[ti[0] − idx_base], Z[ti[0] − idx_base][0..d)} (zeros for ti[0] < 0): a device's pick
// record of one greedy q-EI sub-step, 3 + d doubles
hipError_t launch_pick_record(const double* tv, const int64_t* ti, int64_t idx_base, const double* Z, const double* mu, int d,
                              double* rec, hipStream_t s);

// ---- block form of greedy q-EI (qei.hip): covariance columns of T points from ONE pass over the resident K_ZX ----------
constexpr int QEI_MAXQ = 64;       // picks of one batch (chain vectors kept; their coefficients travel as kernel arguments)
constexpr int QEI_MAXT = 64;       // points of one block (the skinny product holds at most four 16-row groups)
// KXT[t][i] = sigma_f2·kappa(‖Xs_i − s·P_t‖²) for i < N, t < T; zeros for N ≤ i < Np and for T ≤ t < rows.  P: raw points [T][d]
hipError_t launch_qei_kxt(const double* Xs, int dp, int N, int Np, const double* P, int d, int T, int rows, int family, double s,
                          double sigma_f2, double* KXT, hipStream_t st);
// V[r][N … Np) = 0 for r < rows (V: [rows][ld])
hipError_t launch_qei_zero_tail(double* V, int64_t ld, int N, int Np, int rows, hipStream_t st);
// C[t][j] += sigma_f2·kappa(‖Ps_t − s·z_j‖²) for t < T, j < M   (Ps: the block points pre-scaled, [T][dp]; C: [T][Mp])
hipError_t launch_qei_cov(const double* Ps, int dp, const double* Z, int64_t M, int64_t Mp, int d, int T, int family, double s,
                          double sigma_f2, double* C, hipStream_t st);
// C[r][j] = alpha·Σ_{k<K} A[r][k]·B[j][k], r < rows16 (16 … 64, a multiple of 16), j < nB (a multiple of 128), K a multiple of 128:
// the one pass over a long B (gemm.hip: qei_pass_kernel; same bits as the skinny split-k kernel with one chunk)
// kmode K_B_LOWER / K_B_UPPER with ksplit (a multiple of 128): the split-k form against a triangular B — chunk z of the k range of B's row
// block tj → the partial product C + z·sC (launch_splitk_reduce sums them)
hipError_t launch_qei_pass(const double* A, int64_t lda, int rows16, const double* B, int64_t ldb, int64_t nB, int K, double alpha,
                           double* C, int64_t ldc, hipStream_t s, int kmode = K_FULL, int ksplit = 0, int64_t sC = 0);
// out[j] = blk[j] − Σ_{first ≤ i < nchain} gam[i]·chain[i][j] ;  var[j] −= out[j]²/s  (var == nullptr: the column only)
struct QeiPickArgs {
    const double* blk;      // [M]   base covariances of the picked point (a row of the block)
    const double* chain;    // [nchain][Mp]
    double* out;            // [M]   usually chain + nchain·Mp
    double* var;            // [M] or nullptr
    int64_t M, Mp;
    int first, nchain;      // chain entries first … nchain − 1 correct the block's column
    double s;
    double gam[QEI_MAXQ];
};
hipError_t launch_qei_pick(const QeiPickArgs& a, hipStream_t st);
// rec[e] = {tv[e], (double)ti[e], mu, var, Z[0..d), chain_0 … chain_{nchain−1}} of the candidate ti[e] − idx_base (zeros behind a
// negative index), e < k; 4 + d + nchain doubles per record
hipError_t launch_qei_record(const double* tv, const int64_t* ti, int k, int64_t idx_base, const double* Z, const double* mu,
                             const double* var, const double* chain, int64_t Mp, int nchain, int d, double* rec, hipStream_t st);

// ---- the pick loop of a block-form batch on ONE handle, without the host (qei.hip: qei_step_kernel; ABI 7) -------------------------
// Launch k of a batch of q picks (k = 0 … q) finishes pick k − 1 and selects pick k:
//   (B) every workgroup reduces the ≤ QEI_STEP_MAXWG partial arg-maxima launch k − 1 left (strict total order: any reduction tree
//       gives the same winner), workgroup 0 writes the pick's record, every workgroup looks the winner up in the slot table, forms
//       s = σ²(x) + σ²_n and γ_i = c_i(x)/s_i and applies c = C₀[slot] − Σ γ_i c_i, σ² −= c²/s to its candidates (the arithmetic of
//       qei_pick_kernel), then
//   (C) scores its candidates (EI) and leaves its partial arg-max {key, index, μ, σ²} for launch k + 1.
// Launch 0 also snapshots (μ, σ²) — it reads them anyway —, the tail launch (k = q) writes the last record and rolls them back: the
// batch needs no copy of its own before or behind it.
// No workgroup waits for another inside a launch (stream order is the only synchronisation): no atomics, no fences — bit-reproducible.
// A pick outside every block, or s ≤ 0, raises st->stop: the remaining launches return at once, the host builds the block (or reports
// the failed pivot) and resumes from launch k.
constexpr int QEI_STEP_MAXWG = 1024;
struct QeiStepState {                    // device memory, one per candidate set
    int32_t stop;                        // 0: running; 1: pick stop_at is in no block; 2: s ≤ 0 at pick stop_at
    int32_t stop_at;
    double s_batch[QEI_MAXQ];            // s of the picks this batch conditioned on (entry t: the batch's pick t)
};
struct QeiStepPartial { uint64_t key; int64_t idx; double mu, var; };
struct QeiStepArgs {
    double* mu; double* var;             // [M] stored posterior of the set (σ² is conditioned in place; the batch rolls it back)
    double* snap_mu; double* snap_var;   // [M] launch 0 copies (μ, σ²) here, the tail launch (k = q) copies them back
    const double* Z;                     // [M][d]
    const double* blk;                   // [slots][Mp] block columns
    double* chain;                       // [rows][Mp]
    QeiStepState* st;
    QeiStepPartial* part;                // [2][QEI_STEP_MAXWG]: launch k writes half k & 1, reads half (k − 1) & 1
    double* rec;                         // [q][wmax] records {EI, global index, μ, σ², x[d], c_1(x) … c_n(x)}
    int64_t M, Mp, idx_base;
    int d, T16, nslots, wmax;
    int k, q;                            // this launch; picks of the batch
    int n0;                              // chain entries when the batch's pick 0 was selected (real entries carried over)
    int nwg_prev;                        // workgroups of launch k − 1 (partials to reduce)
    int distinct;
    double xi, best_y, noise;
    double chain_s0[QEI_MAXQ];           // s_i of the chain entries i < n0 (host knows them)
    int blk_base[4];                     // per block: chain entries already in its columns
    int64_t slot_gidx[4 * QEI_MAXT];     // global candidate index per block row (−1: empty)
};
hipError_t launch_qei_step(const QeiStepArgs& a, int nwg, hipStream_t st);

// out[0] = max_s min_i ‖S_s − X_i‖ (out: one double in device memory)
hipError_t launch_fill_distance(const double* X, int64_t N, int d, const double* S, int64_t ns, double* out, hipStream_t s);
// Z[(j−j0)·d + c] for j in [j0, j0+count): Latin-hypercube points of an n-point design (device lower/upper)
hipError_t launch_lhs(double* Z, int64_t n, int d, const double* lower, const double* upper, uint64_t seed, int64_t j0,
                      int64_t count, hipStream_t s);

// ---- objectives of the acquisition stage: a weighted sum of epilogues on ONE posterior evaluation ------------------
// f(x) = Σ_t w_t · acq_t(x)  (EnsembleAcquisition, EnsembleAcq.jl:53-55; a plain acquisition function is one term of weight 1).
// acq_t ∈ {EI, UCB, PI, MEAN, LOGEI} on the function-value posterior (μ, σ²), or GRADNORM_UCB on the posterior of the gradient outputs
// of a gradient-enhanced model (gradNormUCB.jl:43-51).
constexpr int MAX_TERMS = 8;
constexpr int ACQ_GRADNORM_UCB = 4;            // == ABO_ACQ_GRADNORM_UCB (include/abo_hip.h)
constexpr int ACQ_LOGEI = 5;                   // == ABO_ACQ_LOGEI
// max-value entropy search (== ABO_ACQ_MES): the one epilogue whose parameter is a VECTOR, the samples y*₀ … y*_{S−1} of the minimum
// value, so it is no kind of the scalar entry points (plain_kind) and no member of an ensemble (acq.hip: make_terms): an objective is
// MES exactly when it is the single term built by the abo_*_mes entry points (terms_mes)
constexpr int ACQ_MES = 6;
constexpr int MES_MAX_SAMPLES = 1024;          // 8 KiB of LDS in the scoring kernel
// the kinds of the entry points that take ONE kind: the epilogues on (μ, σ²) — EI, UCB, PI, MEAN (0 … 3) and LOGEI
inline bool plain_kind(int kind) { return (kind >= 0 && kind < ACQ_GRADNORM_UCB) || kind == ACQ_LOGEI; }
struct AcqTerms {
    int n;
    int kind[MAX_TERMS];
    double p0[MAX_TERMS], best_y[MAX_TERMS], w[MAX_TERMS];
    const double* ystar;                       // ACQ_MES: the samples (device memory) and their number; null / 0 otherwise
    int n_ystar;
};
inline bool terms_mes(const AcqTerms& t) { return t.n == 1 && t.kind[0] == ACQ_MES; }
inline bool terms_have_gradnorm(const AcqTerms& t) {
    for (int i = 0; i < t.n; ++i) if (t.kind[i] == ACQ_GRADNORM_UCB) return true;
    return false;
}
// one term of weight 1 that the fused posterior + epilogue pass scores (MES runs on the μ, σ² of a posterior pass instead)
inline bool terms_plain(const AcqTerms& t) { return t.n == 1 && t.w[0] == 1.0 && t.kind[0] != ACQ_GRADNORM_UCB && t.kind[0] != ACQ_MES; }
// score[j] = Σ_t w_t·acq_t(mu[j], var[j]) (function-value terms only)
hipError_t launch_score_terms(const double* mu, const double* var, double* score, int64_t M, const AcqTerms& t, hipStream_t s);
// score[j] = MES(mu[j], var[j]) = (1/S)·Σ_s a((mu[j] − ystar[s])/σ_j), summed in the order s = 0 … S − 1 (abo_acq_dev.h: mes_a); one lane per
// candidate, the samples staged in LDS; 1 ≤ S ≤ MES_MAX_SAMPLES.  dmu / dvar (both or neither): its partial derivatives as well
hipError_t launch_score_mes(const double* mu, const double* var, int64_t M, const double* ystar, int S, double* score, double* dmu,
                            double* dvar, hipStream_t s);
// gradient-enhanced model: score[j] from the per-point mean mu[j][p] and covariance block cov[j][p][p]
hipError_t launch_score_terms_grad(const double* mu, const double* cov, double* score, int64_t M, int p, const AcqTerms& t, hipStream_t s);

// ---- local refinement of optimize_acquisition on the device (refine.hip) ---------------------------------------
struct RefineArgs {
    const double* Xs;      // [Np][dp] scaled training points
    const double* W;       // L⁻¹ (lower), WT = its transpose (upper); leading dimension ld
    const double* WT;
    const double* alpha;   // [Np]
    int64_t ld;
    int N, Np, d, dp, family;
    double s, sigma_f2, mean_c;            // 1/ℓ, σ_f², prior mean
    AcqTerms terms;                        // the objective
    const double* lower;   // device [d]
    const double* upper;   // device [d]
    const double* starts;  // device [S][d]
    double* x_out;         // device [S][d]   (grad_only: the gradient)
    double* f_out;         // device [S]
    int* iters_out;        // device [S][2] = {iterations, evaluations} or nullptr
    double* scratch;       // device [S][4][Np]
    int max_iter, ls_max, history;
    double g_tol, f_abstol, x_abstol;
};
size_t refine_lds_bytes(int d, int dp, int history);
// one workgroup per start: the whole projected L-BFGS of that start in one launch (grad_only = 1: one evaluation per point,
// x_out receives the gradient)
hipError_t launch_refine(const RefineArgs& a, int S, int grad_only, hipStream_t s);
// the same refinement in lockstep rounds with the evaluations of a round batched on the fp64 MFMA tile core (large N: L⁻¹ is read
// once per round instead of once per start); work = refine_lockstep_bytes(S, Np, d, history) of device memory
size_t refine_lockstep_bytes(int S, int Np, int d, int history);
hipError_t launch_refine_lockstep(const RefineArgs& a, int S, void* work, hipStream_t s);
// Gradient-enhanced models (and any objective with a GRADNORM_UCB term): the same lockstep state machine, a round's evaluations
// delivered by the caller.  eval(points [npts][d] (device), npts, mu [npts][p], cov [npts][p][p]) queues the all-output posterior of
// the round's points on the stream (posterior.hip: the kernels behind abo_predict_grad_cov); the driver derives value and gradient of the
// objective from it — function-value terms analytically (∇μ = E[∇f] − m_∇, ∇σ² = 2·Cov(f, ∇f)), GRADNORM_UCB terms by central
// differences over a 2d-point stencil evaluated in the same batch (the reference differentiates every objective that way,
// acq_utils.jl:55-71).  p = d + 1 outputs; mean_g[d]: prior means of the gradient outputs.
size_t refine_lockstep_grad_bytes(int S, int d, int history, bool stencil);
struct GradEval {
    void* ctx;
    hipError_t (*eval)(void* ctx, const double* pts, int npts, double* mu, double* cov, hipStream_t s);
};
hipError_t launch_refine_lockstep_grad(const RefineArgs& a, int S, const double* mean_g, void* work, const GradEval& ev, hipStream_t s);
// value and gradient of the objective at S points through the same evaluation (the test hook behind abo_test_acq_grad)
hipError_t launch_acq_grad_via_eval(const RefineArgs& a, int S, const double* mean_g, void* work, const GradEval& ev, hipStream_t s);
// out[j][0..d) = Z[idx[j] − idx_base][0..d) for j < k (zeros for idx[j] < 0): the coordinates of selected candidates
hipError_t launch_gather_points(const double* Z, const int64_t* idx, int64_t idx_base, int k, int d, double* out, hipStream_t s);

// ---- pruned top-k selection (misc.hip): candidates whose guarded upper bound reaches the threshold, compacted in index order ----------
// Margins of the guard ub + |ub|·PRUNE_REL + abs_margin (derivation: misc.hip, prune_keep); abs_margin = PRUNE_ABS for EI and UCB,
// PRUNE_ABS_LOGEI for the log-valued LOGEI, whose error does not vanish with the score
constexpr double PRUNE_REL = 0x1p-30;
constexpr double PRUNE_ABS = 0x1p-1022;
constexpr double PRUNE_ABS_LOGEI = 0x1p-30;
constexpr int PRUNE_SCAN_E = 1024;       // candidates per workgroup of the compaction
// sel[0 … *count) = the indices j < M, ascending, with !(guard(ub[j], abs_margin) < *tau) — a NaN on either side keeps the candidate, as the
// selection's order ranks NaN first; *count = their number.  blk: ⌈M / PRUNE_SCAN_E⌉ ints of scratch; sel: room for M entries.
// Stream-ordered, no atomics: the same list on every run.
hipError_t launch_prune_compact(const double* ub, int64_t M, const double* tau, double abs_margin, int* blk, int64_t* sel, int64_t* count,
                                hipStream_t s);
// ub[sel[i]] = min(ub[sel[i]], ub2[i]) for i < n, a NaN on either side giving NaN (kept, as above): the second bound level's tighter
// bounds of the first level's survivors, written back into the bounds of all candidates.  sel: distinct indices (a compacted list).
hipError_t launch_prune_min_scatter(double* ub, const int64_t* sel, const double* ub2, int64_t n, hipStream_t s);
// top_idx[e] = sel[top_idx[e]] + idx_base for e < k (−1 stays): positions in a compacted list back to candidate indices
hipError_t launch_prune_map(int64_t* top_idx, int k, const int64_t* sel, int64_t idx_base, hipStream_t s);

struct TopkWork {            // scratch sized by topk_workspace_entries()
    uint64_t* keys[2];
    int64_t* idx[2];
};
int64_t topk_workspace_entries(int64_t M, int k);
// Which kernels launch_topk gives a selection of k out of M (== ABO_TOPK_PATH_* of include/abo_hip.h): the one place the choice is
// made — pure host code, no GPU call (misc.hip documents the rule)
enum TopkPath {
    TOPK_PATH_NONE = -1,       // k ≤ 0: nothing to do
    TOPK_PATH_SMALL = 0,       // topk_small_kernel<0>: the whole batch in one workgroup's radix select
    TOPK_PATH_SLICES = 1,      // topk_small_kernel<1> per slice, then one merge by topk_small_kernel<2>
    TOPK_PATH_ARGMAX = 2,      // argmax_partial_kernel + argmax_final_kernel (k = 1)
    TOPK_PATH_BLOCKSORT = 3    // the block-sort chain, in threshold rounds of 1024 for k > 1024
};
struct TopkPlan {
    int path;
    int kreal;                 // entries that come from scores: min(k, max(M, 1)); the rest of the k requested is (NaN, −1)
    int slice;                 // SLICES: scores per workgroup of the first launch
    int64_t pairs;             // SLICES: (key, index) pairs the merge reads
    int rounds;                // BLOCKSORT: ⌈kreal/1024⌉ threshold rounds
    int passes;                // BLOCKSORT: launches of topk_pass_kernel in the first round
};
TopkPlan topk_plan(int64_t M, int k);
// top-k of scores[0..M) in Julia's `sortperm(scores; rev=true)` order; writes k (val, idx) pairs
// (idx + idx_base; tail (NaN, −1) when M < k) to device arrays top_val/top_idx.
hipError_t launch_topk(const double* scores, int64_t M, int k, int64_t idx_base, TopkWork w,
                       double* top_val, int64_t* top_idx, hipStream_t s);

// ---- removal of an observation (remove.hip; abo_remove) ----------------------------------------
constexpr int REMOVE_SCAN_CHUNK = 256;   // elements of a row one scan step takes (four 64-lane sub-blocks)
// Row j out of an N-row factor (N ≥ 2): L′ (lower triangle and the identity diagonal of the padding), WT′ and W′ = WT′ᵀ (the whole
// pad128(N − 1)-square block, zeros outside the triangle, identity in the padding) and α′ [N − 1] into buffers of leading dimension
// ldn ≥ pad128(N − 1); the source (leading dimension ld, rows and columns < N only) is read, never written.
// work: 5·N doubles of scratch; scal = {ω = W[j][j], ρ_m² = B_jj/ω², α_j}: log det′ = log det + log(ω²ρ_m²), δ′ᵀα′ = δᵀα − α_j²/(ω²ρ_m²)
struct RemoveArgs {
    const double* L; const double* WT; const double* alpha;
    int64_t ld;
    double* Ln; double* Wn; double* WTn; double* alpha_n;
    int64_t ldn;
    int N, j;
    double* work; double* scal;
};
hipError_t launch_remove_row(const RemoveArgs& a, hipStream_t s);
// the per-point arrays without the k points idx (device, strictly increasing): Nn = the points that remain.  Xs_n / delta_n may be
// null (then Xs / delta are not read)
hipError_t launch_remove_gather(const int64_t* idx, int k, int64_t Nn, int d, int dp, const double* Xraw, const double* Xs, const double* y,
                                const double* delta, double* Xraw_n, double* Xs_n, double* y_n, double* delta_n, hipStream_t s);

}  // namespace abo
