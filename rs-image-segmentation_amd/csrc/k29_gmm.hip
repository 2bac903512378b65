// K29 — rsseg_gmm_sweep: one expectation-maximisation iteration's pass over feature-planar rasters.  Every counted pixel gets
// the k components' whitened quadratic forms (K22's arithmetic, restated), its responsibilities r_j, and, in the same pass,
// enters every component's WEIGHTED count, sum and sum of products with the integer weight q_j = rint(r_j 2^20).  Exact
// integer sums (include/rsseg.h, restated in tests/gmm_ref.py): the table and the tail do not depend on launch geometry.
//
// A workgroup of 256 threads walks tiles of 256 pixels, one pixel per thread:
//   1  mask and the F plane values of the pixel; NaN -> +0, u_f = v_f 2^plane_exp[f], the range test |u_f| <= 1.  The values
//      stay in registers in the planes' type (FR = 8, 16, 24, 32, 64 slots; rows and columns at or beyond F are skipped by
//      uniform branches, as in k22_gauss.hip).
//   2  g_j for j ascending: d_f, the z_i fma chains, the m fma chain, g_j = m + offset_j.  The model is read through
//      wave-uniform indices (scalar loads).  g_j goes to the pixel's column of an LDS array [k][256] (a per-thread array
//      indexed by j would live in scratch); the strictly smaller g wins, so the lowest j keeps a tie.
//   3  e_j = gmm_exp(-0.5 (g_j - best)) over the column, s their sum, r_j = e_j / s, q_j = rint(r_j 2^20), ll; the outputs.
//      q_j replaces g_j in the column.
//   4  (TABLE) the pixel's float32 values are staged in LDS.  Wave w takes the components j = w, w + 4, ...: it compacts the
//      tile's non-zero q_j into a list of (q, slot) entries (ballot and prefix count; K24's sorted list with a weight, the
//      component being the wave's), then every lane owns table columns (lane, lane + 64, ...) and walks the list once per
//      column: term = fx_bits(q u_a 2^Q, u_b), u_b = 1 for the first moments.  q u_a 2^Q is exact (21 + 24 bits) and the fma
//      rounds the exact product once.  A zero q enters no list, so the work follows the non-zero responsibilities, not k.
//      Path A adds the run's sums to the workgroup's table in LDS (flushed once), Path B straight to the global table.
// Without a table (predict) step 4 and its LDS are not compiled in.  No MFMA: float64 fma chains in a fixed order are the
// contract (k28_svm.hip's header has the argument).
#include <algorithm>
#include <cmath>

#include "keyed_table.h"

#define GM_THREADS 256
#define GM_TILE 256
#define GM_LD (GM_TILE + 1)          // row stride of the staged values
#define GM_WAVES (GM_THREADS / WAVE)
#define GM_MAX_K 32
#define GM_LDS_BUDGET (156 * 1024)   // dynamic LDS of one workgroup (160 KiB per CU, less the static counters)
#define GM_MAX_BLOCKS 2048
#define GM_QBITS 20

struct gm_args {
    const void *plane[RSSEG_MAX_FEATURES];
    double scale[RSSEG_MAX_FEATURES];   // 2^plane_exp[f]
    double two_q;                       // 2^Q
    double two_qm;                      // 2^Q for float32 planes, 1 for uint8 planes: the moments' fraction bits
    const double *mean;                 // device [k][F]
    const double *whiten;               // device [k][F (F + 1) / 2]
    const double *offset;               // device [k]
    const uint8_t *mask;
    uint8_t *labels;
    float *posterior, *loglik, *proba;
    int64_t n;
    int F, k;
};

static inline int gm_fr(int F) { return F <= 8 ? 8 : F <= 16 ? 16 : F <= 24 ? 24 : F <= 32 ? 32 : 64; }
static inline int gm_cols(int F, int diag) { return diag ? 1 + 2 * F : 1 + F + F * (F + 1) / 2; }
static inline size_t gm_col_bytes(int k) { return (size_t)k * GM_TILE * 8; }
// staged values (F planes and the row of ones), column look-up (uint16, padded to 8 bytes), scales (F + 1), the waves' lists
static inline size_t gm_acc_bytes(int F, int diag)
{
    const size_t lut = (((size_t)gm_cols(F, diag) - 1) * 2 + 7) & ~(size_t)7;
    return (size_t)(F + 1) * GM_LD * 4 + 4 /* to 8 bytes */ * ((F + 1) & 1) + lut + (size_t)(F + 1) * 8 + (size_t)GM_WAVES * GM_TILE * 4;
}
static inline int gm_path(int F, int k, int diag)   // 0: Path A (table in LDS), 1: Path B
{
    return (size_t)k * gm_cols(F, diag) * 8 + gm_col_bytes(k) + gm_acc_bytes(F, diag) <= GM_LDS_BUDGET ? 0 : 1;
}

// exp(t) for t <= 0: K28's svm_exp, the same operation sequence (include/rsseg.h)
__device__ __forceinline__ double gmm_exp(double t)
{
    const double LOG2E = __longlong_as_double(0x3FF71547652B82FEll), LN2_HI = __longlong_as_double(0x3FE62E42FEE00000ll),
                 LN2_LO = __longlong_as_double(0x3DEA39EF35793C76ll);
    const bool under = t < -708.0;
    const double tc = under ? -708.0 : t;
    const double n = rint(tc * LOG2E);
    double r = fma(-n, LN2_HI, tc);
    r = fma(-n, LN2_LO, r);
    constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                              1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    double p = c[13];
#pragma unroll
    for (int j = 12; j >= 0; j--) p = fma(p, r, c[j]);
    const double two_n = __longlong_as_double((long long)((int)n + 1023) << 52);
    return under ? 0.0 : p * two_n;
}

// ln(s) for s in [1, 64] as a fixed sequence of float64 operations (include/rsseg.h)
__device__ __forceinline__ double gmm_log(double s)
{
    const double LN2_HI = __longlong_as_double(0x3FE62E42FEE00000ll), LN2_LO = __longlong_as_double(0x3DEA39EF35793C76ll),
                 SQRT2 = __longlong_as_double(0x3FF6A09E667F3BCDll);
    constexpr long long LG[7] = {0x3FE5555555555593ll, 0x3FD999999997FA04ll, 0x3FD2492494229359ll, 0x3FCC71C51D8E78AFll,
                                 0x3FC7466496CB03DEll, 0x3FC39A09D078C69Fll, 0x3FC2F112DF3E5244ll};
    const long long bits = __double_as_longlong(s);
    int e = (int)(bits >> 52) - 1023;
    double m = __longlong_as_double((bits & 0x000FFFFFFFFFFFFFll) | 0x3FF0000000000000ll);
    if (m > SQRT2) {
        m = m * 0.5;
        e = e + 1;
    }
    const double f = m - 1.0;
    const double t = f / (2.0 + f);
    const double z = t * t;
    double R = __longlong_as_double(LG[6]);
#pragma unroll
    for (int i = 5; i >= 0; i--) R = fma(R, z, __longlong_as_double(LG[i]));
    R = R * z;
    const double hfsq = (0.5 * f) * f;
    const double dk = (double)e;
    return dk * LN2_HI - ((hfsq - (t * (hfsq + R) + dk * LN2_LO)) - f);
}

// K22's whitened quadratic form (gc_form of k22_gauss.hip, restated for one pixel per lane with u_f = x_f scale_f): rows in
// blocks of RB whose z stay open while the columns go by in blocks of RB, every z_i summed f ascending, m summed i ascending.
// DIAG evaluates the diagonal of W alone: the skipped terms are fma(0, d, z) = z.
template <typename PT, int FR, bool DIAG>
__device__ __forceinline__ double gm_form(const PT (&x)[FR], const gm_args &a, int F, const double *__restrict__ mu, const double *__restrict__ w)
{
    constexpr int RB = FR > 32 ? 32 : FR;
    double m = 0.0;
    if constexpr (DIAG) {
#pragma unroll
        for (int i = 0; i < FR; i++) {
            if (i < F) {
                double u = (double)x[i];
                if (std::is_same<PT, float>::value) u = u * a.scale[i];
                const double d = u - mu[i];
                const double z = fma(w[(i * (i + 1)) / 2 + i], d, 0.0);
                m = fma(z, z, m);
            }
        }
        return m;
    } else {
#pragma unroll
        for (int rb = 0; rb < FR; rb += RB) {
            if (rb < F) {
                double z[RB];
#pragma unroll
                for (int r = 0; r < RB; r++) z[r] = 0.0;
#pragma unroll
                for (int cb = 0; cb <= rb; cb += RB) {
                    double d[RB];
#pragma unroll
                    for (int c = 0; c < RB; c++) {
                        if (cb + c < F) {
                            double u = (double)x[cb + c];
                            if (std::is_same<PT, float>::value) u = u * a.scale[cb + c];
                            d[c] = u - mu[cb + c];
                        } else {
                            d[c] = 0.0;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < RB; r++) {
                        const int i = rb + r;
                        if (i < F) {
                            const double *__restrict__ wrow = w + (i * (i + 1)) / 2 + cb;
#pragma unroll
                            for (int c = 0; c < RB; c++) {
                                if (cb + c <= i) z[r] = fma(wrow[c], d[c], z[r]);   // compile time
                            }
                            if (cb == rb) m = fma(z[r], z[r], m);   // the row is complete: i ascending
                        }
                    }
                }
            }
        }
        return m;
    }
}

// PT: plane element (float, uint8_t); FR: register slots; DIAG: diagonal W and the 1 + 2 F table; MODE 0: no table, 1: Path
// A, 2: Path B
template <typename PT, int FR, bool DIAG, int MODE>
__global__ __launch_bounds__(GM_THREADS) void gmm_sweep(gm_args a, unsigned long long *__restrict__ g_table,
                                                         unsigned long long *__restrict__ g_tail /* counted, left out, far, ll_sum */)
{
    constexpr bool TABLE = MODE != 0, GLOBAL = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char gm_lds[];
    const int F = a.F, k = a.k, tri = (F * (F + 1)) / 2;
    const int C = DIAG ? 1 + 2 * F : 1 + F + tri, NC = C - 1;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / WAVE;
    // dynamic LDS: [table: k * C u64 (Path A)] [col: k * 256 f64: g, then e, then q] [vals: (F + 1) * GM_LD float, row F ones]
    //              [lscale: F + 1 f64] [list: GM_WAVES * 256 u32 = q << 8 | slot] [lut: NC u16 = a << 8 | b]
    unsigned long long *l_table = reinterpret_cast<unsigned long long *>(gm_lds);
    double *col = reinterpret_cast<double *>(gm_lds + (MODE == 1 ? (size_t)k * C * 8 : 0));
    unsigned char *after = reinterpret_cast<unsigned char *>(col + (size_t)k * GM_TILE);
    double *lscale = reinterpret_cast<double *>(after);
    uint32_t *list = reinterpret_cast<uint32_t *>(lscale + (F + 1));
    float *vals = reinterpret_cast<float *>(list + GM_WAVES * GM_TILE);
    uint16_t *lut = reinterpret_cast<uint16_t *>(vals + (size_t)(F + 1) * GM_LD + ((F + 1) & 1));
    if (TABLE) {
        if (MODE == 1) kt_table_zero<GM_THREADS>(l_table, k * C);
        for (int c = tid; c < NC; c += GM_THREADS) {
            int ca = c, cb = F;   // a first moment: u_a times the row of ones
            if (c >= F) {
                if (DIAG) {
                    ca = cb = c - F;
                } else {   // the row-major upper triangle, a <= b
                    int idx = c - F;
                    ca = 0;
                    while (idx >= F - ca) {
                        idx -= F - ca;
                        ca++;
                    }
                    cb = ca + idx;
                }
            }
            lut[c] = (uint16_t)((ca << 8) | cb);
        }
        for (int f = tid; f <= F; f += GM_THREADS) lscale[f] = f < F ? a.scale[f] : 1.0;
        vals[F * GM_LD + tid] = 1.0f;
        __syncthreads();
    }

    unsigned long long n_counted = 0, n_left = 0, n_far = 0, ll_sum = 0;
    const float qnan = __uint_as_float(0x7fc00000u);
    const int64_t ntiles = (a.n + GM_TILE - 1) / GM_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * GM_TILE + tid;
        // ---- 1: mask, values
        const bool inside = i < a.n;
        const bool counted = inside && (a.mask ? a.mask[i] != 0 : true);
        bool kept = false;
        int win = -1;
        double best = (double)INFINITY;
        if (__syncthreads_or(counted)) {   // a tile without a counted pixel reads no feature plane
            PT x[FR];
#pragma unroll
            for (int f = 0; f < FR; f++) x[f] = counted && f < F ? reinterpret_cast<const PT *>(a.plane[f])[i] : (PT)0;
            bool ok = true;
#pragma unroll
            for (int f = 0; f < FR; f++) {
                if (f < F) {
                    if (std::is_same<PT, float>::value) {
                        if (x[f] != x[f]) x[f] = (PT)0;
                        ok = ok && fabs((double)x[f] * a.scale[f]) <= 1.0;
                    }
                    if (TABLE) vals[f * GM_LD + tid] = (float)x[f];
                }
            }
            kept = counted && ok;
            // ---- 2: the quadratic forms
            if (kept) {
                for (int j = 0; j < k; j++) {
                    const double m = gm_form<PT, FR, DIAG>(x, a, F, a.mean + (size_t)j * F, a.whiten + (size_t)j * tri);
                    const double g = m + a.offset[j];
                    col[j * GM_TILE + tid] = g;
                    if (g < best) {
                        best = g;
                        win = j;
                    }
                }
                kept = best < (double)INFINITY && best > -(double)INFINITY;
            }
            if (counted && !kept) n_left++;
            // ---- 3: responsibilities
            double r_win = 0.0, ll = 0.0;
            if (kept) {
                double s = 0.0;
                for (int j = 0; j < k; j++) {
                    const double e = gmm_exp(-0.5 * (col[j * GM_TILE + tid] - best));
                    s = s + e;
                    col[j * GM_TILE + tid] = e;
                }
                for (int j = 0; j < k; j++) {
                    const double r = col[j * GM_TILE + tid] / s;
                    if (j == win) r_win = r;
                    if (a.proba) a.proba[(size_t)j * a.n + i] = (float)r;
                    if (TABLE) reinterpret_cast<unsigned long long *>(col)[j * GM_TILE + tid] = (unsigned long long)(long long)rint(r * (double)(1 << GM_QBITS));
                }
                ll = fma(-0.5, best, gmm_log(s));
                n_counted++;
                if (fabs(ll) < 1048576.0) ll_sum += (unsigned long long)fx_round(ll, a.two_q);
                else n_far++;
            } else {
                if (TABLE)
                    for (int j = 0; j < k; j++) reinterpret_cast<unsigned long long *>(col)[j * GM_TILE + tid] = 0;
                if (inside && a.proba)
                    for (int j = 0; j < k; j++) a.proba[(size_t)j * a.n + i] = qnan;
            }
            if (inside) {
                if (a.labels) a.labels[i] = kept ? (uint8_t)(win + 1) : (uint8_t)0;
                if (a.posterior) a.posterior[i] = kept ? (float)r_win : qnan;
                if (a.loglik) a.loglik[i] = kept ? (float)ll : qnan;
            }
            if (TABLE) {
                // ---- 4: per component, the list of its non-zero weights, then the columns
                __syncthreads();
                unsigned long long *table = GLOBAL ? g_table : l_table;
                uint32_t *mine = list + wave * GM_TILE;
                for (int j0 = 0; j0 < k; j0 += GM_WAVES) {   // the same trip count in every wave: the barriers are uniform
                    const int j = j0 + wave;
                    int cnt = 0;
                    unsigned long long qsum = 0;
                    if (j < k) {
#pragma unroll
                        for (int c = 0; c < GM_TILE / WAVE; c++) {
                            const int p = c * WAVE + lane;
                            const uint32_t q = (uint32_t)reinterpret_cast<const unsigned long long *>(col)[j * GM_TILE + p];
                            const unsigned long long bal = __ballot(q != 0);
                            if (q) mine[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = (q << 8) | (uint32_t)p;
                            cnt += __popcll(bal);
                            qsum += q;
                        }
                    }
                    __syncthreads();   // the list is written
                    if (j < k && cnt > 0) {
                        unsigned long long *row = table + (size_t)j * C;
                        for (int c = lane; c < NC; c += WAVE) {
                            const int ab = lut[c], ca = ab >> 8, cb = ab & 255;
                            const double sa = lscale[ca] * a.two_qm, sb = lscale[cb];
                            const float *va = vals + ca * GM_LD, *vb = vals + cb * GM_LD;
                            unsigned long long acc = 0;
                            for (int e = 0; e < cnt; e++) {
                                const uint32_t ent = mine[e];
                                const int p = (int)(ent & 255u);
                                const double q = (double)(ent >> 8);
                                acc += fx_bits(q * ((double)va[p] * sa), (double)vb[p] * sb);
                            }
                            acc -= fx_bias((unsigned long long)cnt);
                            if (acc) atomicAdd(&row[1 + c], acc);
                        }
                        qsum = wave_sum(qsum);
                        if (lane == 0) atomicAdd(&row[0], qsum);
                    }
                    __syncthreads();   // the next component overwrites the list; the next tile the columns and the values
                }
            }
        } else if (inside) {
            if (a.labels) a.labels[i] = 0;
            if (a.posterior) a.posterior[i] = qnan;
            if (a.loglik) a.loglik[i] = qnan;
            if (a.proba)
                for (int j = 0; j < k; j++) a.proba[(size_t)j * a.n + i] = qnan;
        }
    }
    if (MODE == 1) {
        __syncthreads();
        kt_table_flush<GM_THREADS>(l_table, g_table, k * C);
    }
    n_counted = wave_sum(n_counted);
    n_left = wave_sum(n_left);
    n_far = wave_sum(n_far);
    ll_sum = wave_sum(ll_sum);
    if (lane == 0) {
        if (n_counted) atomicAdd(&g_tail[0], n_counted);
        if (n_left) atomicAdd(&g_tail[1], n_left);
        if (n_far) atomicAdd(&g_tail[2], n_far);
        if (ll_sum) atomicAdd(&g_tail[3], ll_sum);
    }
}

namespace {

template <typename PT, int FR, bool DIAG>
int gm_launch3(rsseg_ctx *ctx, int mode, const gm_args &a, int grid, size_t lds, unsigned long long *table, unsigned long long *tail)
{
    const dim3 g(grid), b(GM_THREADS);
    if (mode == 0) return kt_launch(ctx, gmm_sweep<PT, FR, DIAG, 0>, g, b, lds, a, table, tail);
    if (mode == 1) return kt_launch(ctx, gmm_sweep<PT, FR, DIAG, 1>, g, b, lds, a, table, tail);
    // Path B is reached only where the table of 32 components does not fit beside the rest (gm_path): FULL from 17 planes
    // on, DIAG from 33 on
    if constexpr (DIAG ? FR == 64 : FR >= 24) return kt_launch(ctx, gmm_sweep<PT, FR, DIAG, 2>, g, b, lds, a, table, tail);
    return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "gmm_sweep: no Path B kernel for %d register slots", FR);
}
template <typename PT, bool DIAG>
int gm_launch2(rsseg_ctx *ctx, int fr, int mode, const gm_args &a, int grid, size_t lds, unsigned long long *table, unsigned long long *tail)
{
    switch (fr) {
    case 8: return gm_launch3<PT, 8, DIAG>(ctx, mode, a, grid, lds, table, tail);
    case 16: return gm_launch3<PT, 16, DIAG>(ctx, mode, a, grid, lds, table, tail);
    case 24: return gm_launch3<PT, 24, DIAG>(ctx, mode, a, grid, lds, table, tail);
    case 32: return gm_launch3<PT, 32, DIAG>(ctx, mode, a, grid, lds, table, tail);
    default: return gm_launch3<PT, 64, DIAG>(ctx, mode, a, grid, lds, table, tail);
    }
}

}  // namespace

extern "C" void rsseg_gmm_plan(int F, int k, int dtype, int diag, int *path, int *tile_pixels)
{
    (void)dtype;   // both plane types take the same tile
    const bool ok = F >= 1 && F <= RSSEG_MAX_FEATURES && k >= 1 && k <= GM_MAX_K;
    if (path) *path = ok ? gm_path(F, k, diag != 0) : -1;
    if (tile_pixels) *tile_pixels = ok ? GM_TILE : 0;
}

extern "C" int rsseg_gmm_sweep(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n_local, const uint8_t *d_mask,
                               const int *plane_exp, int Q, int k, int diag, const double *mean, const double *whiten, const double *offset,
                               int64_t *d_table, uint8_t *d_labels, float *d_posterior, float *d_loglik, float *d_proba, int64_t *tail)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || F < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: d_planes is empty (F=%d)", F);
    if (k < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: k=%d, must be >= 1", k);
    if (F > RSSEG_MAX_FEATURES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "gmm_sweep: F=%d feature planes, the kernel takes at most %d", F, RSSEG_MAX_FEATURES);
    if (k > GM_MAX_K) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "gmm_sweep: k=%d components, the kernel takes at most %d", k, GM_MAX_K);
    RSCHK(kt_check_dtype(ctx, "gmm_sweep", dtype, "RSSEG_F32 or RSSEG_U8"));
    if (n_local < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: n_local=%lld is negative", (long long)n_local);
    // a term is at most 2^20 2^Q (2^20 255^2 for uint8 planes) and a sum n_local times that: 2^50 and 2^62 are the limits
    if (Q < 0 || Q > 30) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: Q=%d, must be 0 ... 30", Q);
    if (n_local > ((int64_t)1 << (62 - GM_QBITS - Q)))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: n_local=%lld times 2^(20 + Q) (Q=%d) passes 2^62", (long long)n_local, Q);
    if (dtype == RSSEG_U8 && plane_exp) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: RSSEG_U8 planes take plane_exp = NULL");
    if (dtype == RSSEG_U8 && n_local > ((int64_t)1 << 26))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: n_local=%lld RSSEG_U8 pixels times 2^20 255^2 passes 2^62", (long long)n_local);
    if (dtype == RSSEG_F32 && !plane_exp) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: plane_exp is null");
    if (!mean || !whiten || !offset) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: the model (mean, whiten, offset) is missing");
    if (!tail) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: tail is null");
    if (d_table && ((uintptr_t)d_table & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: d_table not 8-byte aligned");
    if (((uintptr_t)d_posterior | (uintptr_t)d_loglik | (uintptr_t)d_proba) & 3)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: d_posterior, d_loglik or d_proba is not aligned to its element");
    const int tri = F * (F + 1) / 2;
    auto finite = [&](const char *what, const double *v, int count) -> int {
        for (int i = 0; i < count; i++)
            if (!std::isfinite(v[i])) return rs_fail(ctx, RSSEG_ERR_INVALID, "gmm_sweep: %s[%d] is not finite", what, i);
        return RSSEG_OK;
    };
    RSCHK(finite("mean", mean, k * F));
    RSCHK(finite("whiten", whiten, k * tri));
    RSCHK(finite("offset", offset, k));
    gm_args a;
    memset(&a, 0, sizeof(a));
    for (int f = 0; f < F; f++) {
        RSCHK(kt_plane_scale(ctx, "gmm_sweep", plane_exp, f, &a.scale[f]));
        if (n_local > 0) RSCHK(kt_check_plane(ctx, "gmm_sweep", d_planes, f, dtype));
        a.plane[f] = d_planes[f];
    }
    a.two_q = std::ldexp(1.0, Q);
    a.two_qm = dtype == RSSEG_F32 ? a.two_q : 1.0;
    a.mask = d_mask;
    a.labels = d_labels;
    a.posterior = d_posterior;
    a.loglik = d_loglik;
    a.proba = d_proba;
    a.n = n_local;
    a.F = F;
    a.k = k;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool dg = diag != 0;
    const int FR = gm_fr(F), C = gm_cols(F, dg);
    // workspace: the tail's four counters, then the model as the kernel reads it (mean, whiten, offset), uploaded in one copy
    const size_t n_mean = (size_t)k * F, n_wh = (size_t)k * tri;
    const size_t model_bytes = 8 * (n_mean + n_wh + (size_t)k);
    RSCHK(ws_reserve(ctx, 32 + model_bytes));
    RSCHK(pin_reserve(ctx, 32 + model_bytes));
    unsigned long long *d_tail = reinterpret_cast<unsigned long long *>(ctx->d_ws);
    double *d_model = reinterpret_cast<double *>(ctx->d_ws + 32);
    double *h_model = reinterpret_cast<double *>(ctx->h_pin + 32);
    memcpy(h_model, mean, 8 * n_mean);
    memcpy(h_model + n_mean, whiten, 8 * n_wh);
    memcpy(h_model + n_mean + n_wh, offset, 8 * (size_t)k);
    HIPCHK(ctx, hipMemsetAsync(d_tail, 0, 32, ctx->stream));
    if (d_table) HIPCHK(ctx, hipMemsetAsync(d_table, 0, 8 * (size_t)k * C, ctx->stream));
    if (n_local > 0) {
        HIPCHK(ctx, hipMemcpyAsync(d_model, h_model, model_bytes, hipMemcpyHostToDevice, ctx->stream));
        a.mean = d_model;
        a.whiten = d_model + n_mean;
        a.offset = d_model + n_mean + n_wh;
        prof_scope ps(ctx, "gmm_sweep");
        const int mode = !d_table ? 0 : gm_path(F, k, dg) == 0 ? 1 : 2;
        const size_t lds = gm_col_bytes(k) + (mode == 0 ? 0 : gm_acc_bytes(F, dg)) + (mode == 1 ? (size_t)k * C * 8 : 0);
        const int grid = (int)std::min<int64_t>(GM_MAX_BLOCKS, ceil_div64(n_local, GM_TILE));
        unsigned long long *table = reinterpret_cast<unsigned long long *>(d_table);
        int rc;
        if (dtype == RSSEG_F32) rc = dg ? gm_launch2<float, true>(ctx, FR, mode, a, grid, lds, table, d_tail)
                                        : gm_launch2<float, false>(ctx, FR, mode, a, grid, lds, table, d_tail);
        else rc = dg ? gm_launch2<uint8_t, true>(ctx, FR, mode, a, grid, lds, table, d_tail)
                     : gm_launch2<uint8_t, false>(ctx, FR, mode, a, grid, lds, table, d_tail);
        RSCHK(rc);
        HIPCHK(ctx, hipGetLastError());
    }
    unsigned long long h[4];
    RSCHK(kt_read(ctx, d_tail, sizeof(h), h));   // waits: the model's upload has left the pinned area as well
    for (int i = 0; i < 4; i++) tail[i] = (int64_t)h[i];
    return RSSEG_OK;
}
