// K26 — rsseg_isodata_sweep: one ISODATA iteration's pass over feature-planar rasters: every counted pixel is assigned to the
// nearest of k centres (float64, one rounding per operation, no fma) and, in the same pass, enters its cluster's count, sum and
// sum of squares per plane.  Exact integer sums (include/rsseg.h, restated in tests/isodata_ref.py): the table, *n_changed and
// *n_left_out do not depend on launch geometry.
//
// A workgroup of 256 threads walks tiles of 256 pixels, one pixel per thread:
//   1  mask, old label and the F plane values of the pixel; NaN -> +0, u_f = v_f 2^plane_exp[f], the range test |u_f| <= 1,
//      z_f = u_f weight[f] kept in registers. The kernel is instantiated for FR = 8, 16, 24, 32, 64 register slots; the slots
//      f >= F hold z = 0 against centre columns of 0, which add t t = +0 to a distance >= 0 and so leave it as it is: the
//      padded loop gives the bits of the F-term loop.
//   2  the k distances, j ascending, the centres (k x FR float64) read from LDS at a wave-uniform address; the strictly smaller
//      distance wins, so the lowest j keeps a tie.  The label byte is rewritten (255: not counted or left out).
//   3  (TABLE) the pixel's float32 values go to LDS and the (label, slot) pairs are counting-sorted by label (LDS histogram,
//      scan, scatter), as in k24_moments step 2
//   4  (TABLE) a wave takes a quarter of the sorted list, run by run: a run of one label ends where the histogram says, so all
//      lanes of the wave are in the same run and the loop over it tests no label.  A lane owns one plane (its sum and its sum of
//      squares: the value is read once) and every S-th pixel of the run, S = 64 / F; the run's two sums leave 64-bit registers
//      for the table: Path A into the workgroup's table in LDS (added to the global table once, when the workgroup ends), Path
//      B, when that table does not fit beside the centres and the staged tile, straight into the global table.  The counts
//      are the histogram itself.
// Every term is fx_bits(x) = rint(x) (|x| <= 2^50) plus the constant that fx_bias takes off once per run; the
// product (u 2^Q) u of two 24-bit significands is exact in float64.  The adds are 64-bit integer atomics: their order cannot
// change the sums.  Without a table (labels only) steps 3 and 4 are not compiled in.
#include <algorithm>

#include "keyed_table.h"

#define ISO_THREADS 256
#define ISO_TILE 256                 // pixels of a tile: one per thread
#define ISO_LD (ISO_TILE + 1)        // row stride of the staged values: the columns' reads of one slot fall on distinct banks
#define ISO_LDS_BUDGET (128 * 1024)  // dynamic LDS of one workgroup on Path A
#define ISO_MAX_BLOCKS 2048

struct iso_args {
    const void *plane[RSSEG_MAX_FEATURES];
    double scale[RSSEG_MAX_FEATURES];    // 2^plane_exp[f]
    double weight[RSSEG_MAX_FEATURES];
    double two_q;                        // 2^Q
    const double *centers;               // device, k x FR, columns f >= F zero
    uint8_t *labels;
    const uint8_t *mask;
    int64_t n;
    int F, k;
};

static inline int iso_fr(int F) { return F <= 8 ? 8 : F <= 16 ? 16 : F <= 24 ? 24 : F <= 32 ? 32 : 64; }
static inline int iso_cols(int F) { return 1 + 2 * F; }
static inline size_t iso_center_bytes(int F, int k) { return (size_t)k * iso_fr(F) * 8; }
static inline size_t iso_tile_bytes(int F) { return (size_t)F * ISO_LD * 4 + (size_t)ISO_TILE * 4; }
static inline int iso_path(int F, int k)   // 0: Path A (table in LDS), 1: Path B
{
    return (size_t)k * iso_cols(F) * 8 + iso_center_bytes(F, k) + iso_tile_bytes(F) <= ISO_LDS_BUDGET ? 0 : 1;
}

// PT: plane element (float, uint8_t); FR: register slots; MODE 0: labels only, 1: Path A, 2: Path B
template <typename PT, int FR, int MODE>
__global__ __launch_bounds__(ISO_THREADS) void isodata_sweep(iso_args a, unsigned long long *__restrict__ g_table,
                                                              unsigned long long *__restrict__ g_tail /* [0] left out, [1] changed */)
{
    constexpr bool TABLE = MODE != 0, GLOBAL = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char iso_lds[];
    __shared__ int s_hist[RSSEG_MAX_CLUSTERS], s_start[RSSEG_MAX_CLUSTERS], s_total;
    const int F = a.F, k = a.k, C = 1 + 2 * F;
    const int tid = threadIdx.x;
    // dynamic LDS: [table: k * C u64 (Path A)] [centres: k * FR f64] [vals: F * ISO_LD float] [sorted: ISO_TILE u32 = label << 16 | slot]
    unsigned long long *l_table = reinterpret_cast<unsigned long long *>(iso_lds);
    double *cen = reinterpret_cast<double *>(iso_lds + (MODE == 1 ? (size_t)k * C * 8 : 0));
    float *vals = reinterpret_cast<float *>(cen + (size_t)k * FR);
    uint32_t *sorted = reinterpret_cast<uint32_t *>(vals + (size_t)F * ISO_LD);
    if (MODE == 1) kt_table_zero<ISO_THREADS>(l_table, k * C);
    for (int i = tid; i < k * FR; i += ISO_THREADS) cen[i] = a.centers[i];
    __syncthreads();

    // the plane and the place in its wave of this thread (step 4)
    const int wave = tid / WAVE, S = WAVE / F;   // S >= 1: F <= 64
    const int sub = lane_id() / F, cf = lane_id() % F;
    const bool active = TABLE && sub < S;
    const double cscale = a.scale[cf], cscale_q = cscale * a.two_q;

    unsigned long long n_left = 0, n_changed = 0;
    const int64_t ntiles = (a.n + ISO_TILE - 1) / ISO_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i = tile * ISO_TILE + tid;
        // ---- 1: mask, old label, values
        const bool inside = i < a.n;
        const bool counted = inside && (a.mask ? a.mask[i] != 0 : true);
        const int old = inside ? (int)a.labels[i] : 255;
        if (TABLE) {
            if (tid < RSSEG_MAX_CLUSTERS) s_hist[tid] = 0;
            if (!__syncthreads_or(counted)) {   // no counted pixel: no feature plane is read
                if (inside && old != 255) a.labels[i] = 255;
                continue;
            }
        }
        PT raw[FR];
#pragma unroll
        for (int f = 0; f < FR; f++) raw[f] = counted && f < F ? reinterpret_cast<const PT *>(a.plane[f])[i] : (PT)0;
        double z[FR];
        bool ok = true;
#pragma unroll
        for (int f = 0; f < FR; f++) {
            float v = (float)raw[f];   // staging, as K24 step 2: NaN -> +0, the range test on the scaled value
            double u = (double)v;
            if (std::is_same<PT, float>::value) {
                if (v != v) v = 0.0f;
                u = (double)v * a.scale[f];
                if (f < F) ok = ok && fabs(u) <= 1.0;
            }
            z[f] = f < F ? u * a.weight[f] : 0.0;
            if (TABLE && f < F) vals[f * ISO_LD + tid] = v;
        }
        const bool kept = counted && ok;
        if (counted && !ok) n_left++;
        // ---- 2: the nearest centre
        int best = 255;
        if (kept) {
            double bd = 0.0;
            for (int j = 0; j < k; j++) {
                const double *c = cen + j * FR;
                double d = 0.0;
#pragma unroll
                for (int f = 0; f < FR; f++) {
                    const double t = z[f] - c[f];
                    d = d + t * t;
                }
                if (j == 0 || d < bd) {
                    bd = d;
                    best = j;
                }
            }
            if (best != old) n_changed++;
        }
        if (inside && best != old) a.labels[i] = (uint8_t)best;
        if (TABLE) {
            // ---- 3: counting sort of the kept pixels by label
            int pos = 0;
            if (kept) pos = atomicAdd(&s_hist[best], 1);
            __syncthreads();
            if (tid < WAVE) {   // exclusive scan of the histogram (64 entries, one wave); wave_incl_scan written out: the helper cost the float32 kernels 0.3 %
                const int h = s_hist[tid];
                int inc = h;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const int up = __shfl_up(inc, o, WAVE);
                    if (tid >= o) inc += up;
                }
                s_start[tid] = inc - h;
                if (tid == WAVE - 1) s_total = inc;
            }
            __syncthreads();
            if (kept) sorted[s_start[best] + pos] = kt_sorted_entry(best, tid);
            __syncthreads();
            // ---- 4: the runs
            const int total = s_total;
            unsigned long long *table = GLOBAL ? g_table : l_table;
            {
                int p = (int)(((long long)wave * total) / (ISO_THREADS / WAVE));
                const int end = (int)(((long long)(wave + 1) * total) / (ISO_THREADS / WAVE));
                while (p < end) {   // wave-uniform: every lane of the wave is in the same run
                    const int cur = kt_entry_label(sorted[p]);
                    const int run_end = min(end, s_start[cur] + s_hist[cur]);
                    if (active) {
                        unsigned long long a1 = 0, a2 = 0;
                        unsigned int cnt = 0;
                        for (int q = p + sub; q < run_end; q += S) {   // no label test inside a run
                            const double v = (double)vals[cf * ISO_LD + kt_entry_slot(sorted[q])];
                            const double x = v * cscale_q;   // u 2^Q: a product with a power of two, exact
                            a1 += fx_bits(x);
                            a2 += fx_bits(x * (v * cscale));
                            cnt++;
                        }
                        const unsigned long long bias = fx_bias(cnt);
                        unsigned long long *row = table + (size_t)cur * C;
                        if (a1 != bias) atomicAdd(&row[1 + cf], a1 - bias);
                        if (a2 != bias) atomicAdd(&row[1 + F + cf], a2 - bias);
                    }
                    p = run_end;
                }
            }
            if (tid < k && s_hist[tid]) atomicAdd(&table[(size_t)tid * C], (unsigned long long)s_hist[tid]);   // the counts are the histogram
            __syncthreads();   // the next tile overwrites the histogram, the values and the list
        }
    }
    if (MODE == 1) {
        __syncthreads();
        kt_table_flush<ISO_THREADS>(l_table, g_table, k * C);
    }
    n_left = wave_sum(n_left);
    n_changed = wave_sum(n_changed);
    if (lane_id() == 0) {
        if (n_left) atomicAdd(&g_tail[0], n_left);
        if (n_changed) atomicAdd(&g_tail[1], n_changed);
    }
}

namespace {

template <typename PT, int FR> int iso_launch2(rsseg_ctx *ctx, int mode, const iso_args &a, int grid, size_t lds, unsigned long long *table, unsigned long long *tail)
{
    const dim3 g(grid), b(ISO_THREADS);
    if (mode == 0) return kt_launch(ctx, isodata_sweep<PT, FR, 0>, g, b, lds, a, table, tail);
    if (mode == 1) return kt_launch(ctx, isodata_sweep<PT, FR, 1>, g, b, lds, a, table, tail);
    // Path B is reached only by the widest stacks: narrower ones always fit the budget (iso_path)
    if (FR == 64) return kt_launch(ctx, isodata_sweep<PT, 64, 2>, g, b, lds, a, table, tail);
    return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "isodata_sweep: no Path B kernel for %d register slots", FR);
}
template <typename PT> int iso_launch1(rsseg_ctx *ctx, int fr, int mode, const iso_args &a, int grid, size_t lds, unsigned long long *table, unsigned long long *tail)
{
    switch (fr) {
    case 8: return iso_launch2<PT, 8>(ctx, mode, a, grid, lds, table, tail);
    case 16: return iso_launch2<PT, 16>(ctx, mode, a, grid, lds, table, tail);
    case 24: return iso_launch2<PT, 24>(ctx, mode, a, grid, lds, table, tail);
    case 32: return iso_launch2<PT, 32>(ctx, mode, a, grid, lds, table, tail);
    default: return iso_launch2<PT, 64>(ctx, mode, a, grid, lds, table, tail);
    }
}

}  // namespace

extern "C" void rsseg_isodata_plan(int F, int k, int dtype, int *path, int *tile_pixels)
{
    (void)dtype;   // both plane types take the same tile
    const bool ok = F >= 1 && F <= RSSEG_MAX_FEATURES && k >= 1 && k <= RSSEG_MAX_CLUSTERS;
    if (path) *path = ok ? iso_path(F, k) : -1;
    if (tile_pixels) *tile_pixels = ok ? ISO_TILE : 0;
}

extern "C" int rsseg_isodata_sweep(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n_local, const uint8_t *d_mask,
                                   const int *plane_exp, int Q, const double *weight, int k, const double *centers, uint8_t *d_labels,
                                   int64_t *d_table, int64_t *n_changed, int64_t *n_left_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || F < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: d_planes is empty (F=%d)", F);
    if (k < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: k=%d, must be >= 1", k);
    if (F > RSSEG_MAX_FEATURES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "isodata_sweep: F=%d feature planes, the kernel takes at most %d", F, RSSEG_MAX_FEATURES);
    if (k > RSSEG_MAX_CLUSTERS) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "isodata_sweep: k=%d clusters, the kernel takes at most %d", k, RSSEG_MAX_CLUSTERS);
    RSCHK(kt_check_dtype(ctx, "isodata_sweep", dtype, "RSSEG_F32 or RSSEG_U8"));
    if (n_local < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: n_local=%lld is negative", (long long)n_local);
    RSCHK(kt_check_fixed(ctx, "isodata_sweep", dtype, plane_exp, Q, n_local));
    if (!weight) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: weight is null");
    if (!centers) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: centers is null");
    if (d_table && ((uintptr_t)d_table & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: d_table not 8-byte aligned");
    if (!n_changed) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: n_changed is null");
    if (!n_left_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: n_left_out is null");
    iso_args a;
    memset(&a, 0, sizeof(a));
    for (int f = 0; f < F; f++) {
        RSCHK(kt_plane_scale(ctx, "isodata_sweep", plane_exp, f, &a.scale[f]));
        if (!std::isfinite(weight[f])) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: weight[%d] is not finite", f);
        a.weight[f] = weight[f];
        if (n_local > 0) RSCHK(kt_check_plane(ctx, "isodata_sweep", d_planes, f, dtype));
        a.plane[f] = d_planes[f];
    }
    for (int j = 0; j < k; j++)
        for (int f = 0; f < F; f++)
            if (!std::isfinite(centers[(size_t)j * F + f]))
                return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: centers[%d][%d] is not finite", j, f);
    if (n_local > 0 && !d_labels) return rs_fail(ctx, RSSEG_ERR_INVALID, "isodata_sweep: d_labels is null");
    a.two_q = std::ldexp(1.0, Q);
    a.labels = d_labels;
    a.mask = d_mask;
    a.n = n_local;
    a.F = F;
    a.k = k;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int FR = iso_fr(F), C = iso_cols(F);
    const size_t cen_bytes = iso_center_bytes(F, k);
    // workspace: {left out, changed}, then the padded centres; pinned: the centres going up, then the two counts coming down
    RSCHK(ws_reserve(ctx, 16 + cen_bytes));
    RSCHK(pin_reserve(ctx, 16 + cen_bytes));
    unsigned long long *tail = reinterpret_cast<unsigned long long *>(ctx->d_ws);
    double *d_cen = reinterpret_cast<double *>(ctx->d_ws + 16);
    double *h_cen = reinterpret_cast<double *>(ctx->h_pin + 16);
    for (int j = 0; j < k; j++)
        for (int f = 0; f < FR; f++) h_cen[(size_t)j * FR + f] = f < F ? centers[(size_t)j * F + f] : 0.0;
    HIPCHK(ctx, hipMemsetAsync(tail, 0, 16, ctx->stream));
    if (d_table) HIPCHK(ctx, hipMemsetAsync(d_table, 0, 8 * (size_t)k * C, ctx->stream));
    if (n_local > 0) {
        HIPCHK(ctx, hipMemcpyAsync(d_cen, h_cen, cen_bytes, hipMemcpyHostToDevice, ctx->stream));
        a.centers = d_cen;
        prof_scope ps(ctx, "isodata_sweep");
        const int mode = !d_table ? 0 : iso_path(F, k) == 0 ? 1 : 2;
        const size_t lds = cen_bytes + (mode == 0 ? 0 : iso_tile_bytes(F)) + (mode == 1 ? (size_t)k * C * 8 : 0);
        const int grid = (int)std::min<int64_t>(ISO_MAX_BLOCKS, ceil_div64(n_local, ISO_TILE));
        unsigned long long *table = reinterpret_cast<unsigned long long *>(d_table);
        if (dtype == RSSEG_F32) RSCHK(iso_launch1<float>(ctx, FR, mode, a, grid, lds, table, tail));
        else RSCHK(iso_launch1<uint8_t>(ctx, FR, mode, a, grid, lds, table, tail));
        HIPCHK(ctx, hipGetLastError());
    }
    unsigned long long h[2];
    RSCHK(kt_read(ctx, tail, sizeof(h), h));
    *n_left_out = (int64_t)h[0];
    *n_changed = (int64_t)h[1];
    return RSSEG_OK;
}
