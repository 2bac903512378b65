// K24 — rsseg_class_moments: per-label sums of 1, x and x x^T over feature-planar rasters (the keyed form of k3_gram).
// Exact integer sums (include/rsseg.h, restated in tests/moments_ref.py): the table does not depend on launch geometry.
//
// The pixel is the augmented vector y = (1, u_0 .. u_{F-1}); the output columns are the row-major upper triangle of y y^T over
// FA = F + 1 entries: (0, 0) the count, (0, 1 + f) the first moments, (1 + a, 1 + b) the products.  Every term is
//   bits(fma(y_a * 2^Q, y_b, FX_MAGIC)) - bits(FX_MAGIC) = rint(y_a * 2^Q * y_b)
// (y_a * 2^Q is exact, the product of two 24-bit significands is exact inside the fma, one rounding to nearest-even), the constant
// taken off once per run as in k3_gram.  The count column therefore sums 2^Q per pixel and is shifted down at the end.
//
// A workgroup walks spans of 4096 pixels (passed over at once when no pixel of the span counts) in tiles of mo_tile(F) pixels:
//   1  labels and mask: which pixels count; a tile without one reads no feature plane
//   2  the counted pixels' values go to LDS (float32, NaN as 0; the power-of-two plane scale is applied in float64 where the
//      value is used), the range test |u_f| <= 1 drops a pixel into *n_left_out, and a counting sort by label (LDS histogram,
//      scan, scatter) leaves a list of (label, slot) in which every label is one run
//   3  a thread owns one 4 x 4 block (rows a0 .. a0 + 3, columns b0 .. b0 + 3, a0 <= b0) of the triangle, so that eight LDS
//      reads feed sixteen fmas, and one of PS contiguous pieces of the sorted list (a piece crosses few label changes); it
//      accumulates a run in 64-bit registers, two pixels at a time while the label holds, and adds the finished run into the
//      table: Path A into the workgroup's table in LDS (added to the global table once, when the workgroup ends), Path B,
//      when that table does not fit, straight into the global table.  A block on the diagonal computes its lower half for
//      nothing and a block at the ragged edge computes columns beyond F (210 of 240 fmas are kept at F = 19, 2145 of 2448
//      at F = 64); neither is added.
// The adds are 64-bit integer atomics: their order cannot change the sums.
#include <algorithm>

#include "keyed_table.h"

#define MO_THREADS 256
#define MO_R 4               // rows and columns of a thread's block
#define MO_MAX_CLASSES 256
#define MO_LDS_BUDGET (96 * 1024)   // dynamic LDS of one workgroup on Path A: the table, the staged tile, the sorted list
#define MO_MAX_BLOCKS 1024
#define MO_LD 8              // planes whose loads are in flight together while a tile is staged
#define MO_SPAN 4096         // pixels a workgroup takes at a time: a multiple of both tile sizes

struct mo_args {
    const void *plane[RSSEG_MAX_FEATURES];
    double scale[RSSEG_MAX_FEATURES];   // 2^plane_exp[f]
    double two_q;                       // 2^Q
    const void *labels;
    const uint8_t *mask;
    int64_t n;
    int F, k, ignore, has_ignore;
};

// pixels a workgroup stages at a time.  Measured at 16384^2 (profiles/moments_bench.json): 256 leaves LDS for four workgroups
// per CU at F = 19 (18.7 ms against 21.4 ms with 512); narrow stacks do so little work per tile that the larger tile's
// fewer barriers and flushes win (7 uint8 planes: 7.9 ms against 10.7 ms)
static inline int mo_tile(int F) { return F <= 8 ? 512 : 256; }
static inline int mo_cols(int F) { return 1 + F + F * (F + 1) / 2; }
static inline int mo_blocks(int F)   // 4 x 4 blocks on and above the diagonal of the (F + 1) x (F + 1) triangle: 153 at F = 64
{
    const int g = (F + 1 + MO_R - 1) / MO_R;
    return g * (g + 1) / 2;
}
static inline size_t mo_tile_bytes(int F) { return (size_t)mo_tile(F) * (4 * (F + 1) + 4); }
static inline int mo_path(int F, int k)   // 0: Path A (table in LDS), 1: Path B
{
    return (size_t)k * mo_cols(F) * 8 + mo_tile_bytes(F) <= MO_LDS_BUDGET ? 0 : 1;
}

// PT: plane element (float, uint8_t); LT: label element (uint8_t, int); GLOBAL: Path B.  B: blocks, PS: pieces, B * PS <= 256
template <typename PT, typename LT, bool GLOBAL>
__global__ __launch_bounds__(MO_THREADS) void class_moments(mo_args a, int T, int B, int PS, unsigned long long *__restrict__ g_table,
                                                             unsigned long long *__restrict__ g_tail /* [0] left out, [1] bad labels */)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mo_lds[];
    __shared__ int s_hist[MO_MAX_CLASSES], s_start[MO_MAX_CLASSES], s_wsum[MO_THREADS / WAVE], s_total;
    __shared__ double s_scale[RSSEG_MAX_FEATURES + 1];
    const int F = a.F, FA = F + 1, k = a.k, C = 1 + F + (F * (F + 1)) / 2;
    const int tid = threadIdx.x;
    // dynamic LDS: [table: k * C u64 (Path A)] [vals: FA * T float] [sorted: T u32 = label << 16 | slot]
    unsigned long long *l_table = reinterpret_cast<unsigned long long *>(mo_lds);
    float *vals = reinterpret_cast<float *>(mo_lds + (GLOBAL ? 0 : (size_t)k * C * 8));
    uint32_t *sorted = reinterpret_cast<uint32_t *>(vals + (size_t)FA * T);
    if (!GLOBAL) kt_table_zero<MO_THREADS>(l_table, k * C);
    if (tid <= F) s_scale[tid] = tid == 0 ? 1.0 : a.scale[tid - 1];
    __syncthreads();

    // the block of this thread: block id -> (block row, block column), row-major over the upper triangle of blocks
    const int piece = tid / B;
    const bool active = piece < PS;
    int a0 = 0, b0 = 0;
    {
        const int g = (FA + MO_R - 1) / MO_R;
        int id = tid % B, row = 0;
        while (id >= g - row) {
            id -= g - row;
            row++;
        }
        a0 = MO_R * row;
        b0 = MO_R * (row + id);
    }
    int ia[MO_R], ib[MO_R];          // LDS rows of the block's rows and columns; beyond F: row F again, never added
    double sa[MO_R], sb[MO_R];       // their plane scales, the rows' times 2^Q
#pragma unroll
    for (int r = 0; r < MO_R; r++) {
        ia[r] = min(a0 + r, F) * T;
        ib[r] = min(b0 + r, F) * T;
        sa[r] = s_scale[min(a0 + r, F)] * a.two_q;
        sb[r] = s_scale[min(b0 + r, F)];
    }
    unsigned long long n_left = 0;
    bool bad = false;
    const int PPT = T / MO_THREADS;   // 1 or 2
    const int64_t ntiles = (a.n + T - 1) / T;
    const LT *__restrict__ labels = reinterpret_cast<const LT *>(a.labels);

    // A workgroup takes spans of MO_SPAN pixels.  Where a label can be ignored or a mask is given, it first looks through the
    // span's labels with all of its loads in flight at once and passes over a span without a counted pixel: a sparse ROI
    // costs one wait per 4096 labels, not one per tile.
    const int64_t nspans = (a.n + MO_SPAN - 1) / MO_SPAN;
    for (int64_t span = blockIdx.x; span < nspans; span += gridDim.x) {
        const int64_t sbase = span * MO_SPAN;
        if (a.has_ignore || a.mask) {
            int lv[MO_SPAN / MO_THREADS];
#pragma unroll
            for (int j = 0; j < MO_SPAN / MO_THREADS; j++) lv[j] = (int)labels[min(sbase + j * MO_THREADS + tid, a.n - 1)];
            bool some = false;
#pragma unroll
            for (int j = 0; j < MO_SPAN / MO_THREADS; j++) {
                const int64_t i = sbase + j * MO_THREADS + tid;
                if (i < a.n && !(a.has_ignore && lv[j] == a.ignore)) some = some || (a.mask ? a.mask[i] != 0 : true);
            }
            if (!__syncthreads_or(some)) continue;
        }
        const int64_t tile_end = min(ntiles, (sbase + MO_SPAN) / T);
        for (int64_t tile = sbase / T; tile < tile_end; tile++) {
            const int64_t base = tile * T;
            // ---- 1: labels and mask
            s_hist[tid] = 0;
            int mylab[2] = {-1, -1};
            bool any = false;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int64_t i = base + j * MO_THREADS + tid;
                if (j < PPT && i < a.n) {
                    const bool m = a.mask ? a.mask[i] != 0 : true;
                    const int l = (int)labels[i];
                    if (m && !(a.has_ignore && l == a.ignore)) {
                        if ((unsigned)l >= (unsigned)k) bad = true;   // never used as an index
                        else mylab[j] = l;
                    }
                }
                any = any || mylab[j] >= 0;
            }
            if (!__syncthreads_or(any)) continue;   // no counted pixel: no feature plane is read
            // ---- 2: stage the counted pixels, drop those out of range, count per label
            int mypos[2] = {0, 0};
            bool ok[2] = {true, true};
            // MO_LD planes of both pixels are loaded before the first is used: the loads of a tile cost F / MO_LD waits, not 2 F
            for (int f0 = 0; f0 < F; f0 += MO_LD) {
                PT raw[2][MO_LD];
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int u = 0; u < MO_LD; u++)
                        raw[j][u] = mylab[j] >= 0 ? reinterpret_cast<const PT *>(a.plane[min(f0 + u, F - 1)])[base + j * MO_THREADS + tid] : (PT)0;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    if (mylab[j] < 0) continue;
#pragma unroll
                    for (int u = 0; u < MO_LD; u++) {
                        if (f0 + u < F) {
                            float v = (float)raw[j][u];   // staging, as K26 step 1: NaN -> +0, the range test on the scaled value
                            if (std::is_same<PT, float>::value) {
                                if (v != v) v = 0.0f;
                                ok[j] = ok[j] && fabs((double)v * a.scale[f0 + u]) <= 1.0;
                            }
                            vals[(size_t)(f0 + u + 1) * T + j * MO_THREADS + tid] = v;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (mylab[j] < 0) continue;
                vals[j * MO_THREADS + tid] = 1.0f;
                if (ok[j]) mypos[j] = atomicAdd(&s_hist[mylab[j]], 1);
                else { mylab[j] = -1; n_left++; }
            }
            __syncthreads();
            {   // exclusive scan of the histogram (256 entries, one per thread); wave_incl_scan written out: the helper changes the kernel's code
                const int h = s_hist[tid];
                int inc = h;
#pragma unroll
                for (int o = 1; o < WAVE; o <<= 1) {
                    const int up = __shfl_up(inc, o, WAVE);
                    if (lane_id() >= o) inc += up;
                }
                if (lane_id() == WAVE - 1) s_wsum[tid >> 6] = inc;
                __syncthreads();
                int before = 0;
                for (int w = 0; w < (tid >> 6); w++) before += s_wsum[w];
                s_start[tid] = before + inc - h;
                if (tid == MO_THREADS - 1) s_total = before + inc;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (mylab[j] >= 0) sorted[s_start[mylab[j]] + mypos[j]] = kt_sorted_entry(mylab[j], j * MO_THREADS + tid);
            __syncthreads();
            // ---- 3: the runs
            const int total = s_total;
            if (active) {
                unsigned long long acc[MO_R][MO_R];
                unsigned long long cnt = 0;
                int cur = -1;
#pragma unroll
                for (int r = 0; r < MO_R; r++)
#pragma unroll
                    for (int c = 0; c < MO_R; c++) acc[r][c] = 0;
                auto flush = [&]() {
                    if (cnt) {
                        const unsigned long long bias = fx_bias(cnt);
                        unsigned long long *row = (GLOBAL ? g_table : l_table) + (size_t)cur * C;
#pragma unroll
                        for (int r = 0; r < MO_R; r++)
#pragma unroll
                            for (int c = 0; c < MO_R; c++) {
                                const int ya = a0 + r, yb = b0 + c;
                                const unsigned long long v = acc[r][c] - bias;
                                if (ya <= yb && yb <= F && v) atomicAdd(&row[ya * FA - (ya * (ya - 1)) / 2 + (yb - ya)], v);
                                acc[r][c] = 0;
                            }
                        cnt = 0;
                    }
                };
                auto pixel = [&](int slot) {
                    double xs[MO_R], xb[MO_R];
#pragma unroll
                    for (int r = 0; r < MO_R; r++) {
                        xs[r] = (double)vals[ia[r] + slot] * sa[r];
                        xb[r] = (double)vals[ib[r] + slot] * sb[r];
                    }
#pragma unroll
                    for (int r = 0; r < MO_R; r++)
#pragma unroll
                        for (int c = 0; c < MO_R; c++) acc[r][c] += fx_bits(xs[r], xb[c]);
                };
                int p = (int)(((long long)piece * total) / PS);
                const int end = (int)(((long long)(piece + 1) * total) / PS);
                while (p < end) {
                    const uint32_t e0 = sorted[p];
                    const uint32_t e1 = sorted[min(p + 1, end - 1)];
                    if (kt_entry_label(e0) != cur) {
                        flush();
                        cur = kt_entry_label(e0);
                    }
                    pixel(kt_entry_slot(e0));
                    cnt++;
                    p++;
                    if (p < end && kt_entry_label(e1) == cur) {   // the next pixel of the same run: its loads overlap the first one's fmas
                        pixel(kt_entry_slot(e1));
                        cnt++;
                        p++;
                    }
                }
                flush();
            }
            __syncthreads();   // the next tile overwrites the histogram, the values and the list
        }
    }
    if (!GLOBAL) {
        __syncthreads();
        kt_table_flush<MO_THREADS>(l_table, g_table, k * C);
    }
    if (n_left) atomicAdd(&g_tail[0], n_left);
    if (bad) atomicAdd(&g_tail[1], 1ull);
}

// the count column summed 2^Q per pixel
__global__ void class_moments_counts(long long *__restrict__ table, int k, int C, int Q)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < k) table[(size_t)j * C] >>= Q;
}

namespace {

template <typename PT, typename LT, typename... A> int mo_launch(rsseg_ctx *ctx, bool global, int grid, size_t lds, A... x)
{
    return kt_launch(ctx, global ? class_moments<PT, LT, true> : class_moments<PT, LT, false>, dim3(grid), dim3(MO_THREADS), lds, x...);
}

}  // namespace

extern "C" void rsseg_class_moments_plan(int F, int n_classes, int dtype, int *path, int *tile_pixels)
{
    (void)dtype;   // both plane types take the same tile
    const bool ok = F >= 1 && F <= RSSEG_MAX_FEATURES && n_classes >= 1 && n_classes <= MO_MAX_CLASSES;
    if (path) *path = ok ? mo_path(F, n_classes) : -1;
    if (tile_pixels) *tile_pixels = ok ? mo_tile(F) : 0;
}

extern "C" int rsseg_class_moments(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n_local, const void *d_labels, int label_dtype,
                                   int n_classes, int ignore, const uint8_t *d_mask, const int *plane_exp, int Q, int64_t *d_out, int64_t *n_left_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || F < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: d_planes is empty (F=%d)", F);
    if (n_classes < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: n_classes=%d, must be >= 1", n_classes);
    if (F > RSSEG_MAX_FEATURES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "class_moments: F=%d feature planes, the kernel takes at most %d", F, RSSEG_MAX_FEATURES);
    if (n_classes > MO_MAX_CLASSES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "class_moments: n_classes=%d, the kernel takes at most %d", n_classes, MO_MAX_CLASSES);
    RSCHK(kt_check_dtype(ctx, "class_moments", dtype, "RSSEG_F32 or RSSEG_U8"));
    if (label_dtype != RSSEG_U8 && label_dtype != RSSEG_I32) return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: label_dtype must be RSSEG_U8 or RSSEG_I32");
    if (n_local < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: n_local=%lld is negative", (long long)n_local);
    RSCHK(kt_check_fixed(ctx, "class_moments", dtype, plane_exp, Q, n_local));
    if (!d_out || ((uintptr_t)d_out & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: d_out null or not 8-byte aligned");
    if (!n_left_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: n_left_out is null");
    mo_args a;
    memset(&a, 0, sizeof(a));
    for (int f = 0; f < F; f++) {
        RSCHK(kt_plane_scale(ctx, "class_moments", plane_exp, f, &a.scale[f]));
        if (n_local > 0) RSCHK(kt_check_plane(ctx, "class_moments", d_planes, f, dtype));
        a.plane[f] = d_planes[f];
    }
    if (n_local > 0 && (!d_labels || (label_dtype == RSSEG_I32 && ((uintptr_t)d_labels & 3))))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: d_labels null or not aligned to its element");
    a.two_q = std::ldexp(1.0, Q);
    a.labels = d_labels;
    a.mask = d_mask;
    a.n = n_local;
    a.F = F;
    a.k = n_classes;
    a.ignore = ignore;
    a.has_ignore = ignore != -1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int C = mo_cols(F);
    const int64_t cells = (int64_t)n_classes * C;
    const size_t table_bytes = sizeof(int64_t) * (size_t)(cells + 2);   // the table, then {left out, bad labels}
    RSCHK(ws_reserve(ctx, table_bytes));
    RSCHK(pin_reserve(ctx, 256));
    unsigned long long *table = reinterpret_cast<unsigned long long *>(ctx->d_ws);
    unsigned long long *tail = table + cells;
    HIPCHK(ctx, hipMemsetAsync(table, 0, table_bytes, ctx->stream));
    if (n_local > 0) {
        prof_scope ps(ctx, "class_moments");
        const int T = mo_tile(F), B = mo_blocks(F), PS = MO_THREADS / B;
        const bool global = mo_path(F, n_classes) != 0;
        const size_t lds = mo_tile_bytes(F) + (global ? 0 : (size_t)cells * 8);
        const int grid = (int)std::min<int64_t>(MO_MAX_BLOCKS, ceil_div64(n_local, MO_SPAN));
        if (dtype == RSSEG_F32) {
            if (label_dtype == RSSEG_U8) RSCHK((mo_launch<float, uint8_t>(ctx, global, grid, lds, a, T, B, PS, table, tail)));
            else RSCHK((mo_launch<float, int>(ctx, global, grid, lds, a, T, B, PS, table, tail)));
        } else {
            if (label_dtype == RSSEG_U8) RSCHK((mo_launch<uint8_t, uint8_t>(ctx, global, grid, lds, a, T, B, PS, table, tail)));
            else RSCHK((mo_launch<uint8_t, int>(ctx, global, grid, lds, a, T, B, PS, table, tail)));
        }
        if (Q > 0)
            hipLaunchKernelGGL(class_moments_counts, dim3((n_classes + 255) / 256), dim3(256), 0, ctx->stream, (long long *)table, n_classes, C, Q);
        HIPCHK(ctx, hipGetLastError());
    }
    // sum over ranks: the table and the left-out count pass through the communication buffer in pieces that fit it
    if (ctx->comm_on) {
        const int64_t total = cells + 1, piece = (int64_t)(ctx->comm_bytes / 8);
        if (piece < 1) return rs_fail(ctx, RSSEG_ERR_COMM, "class_moments: comm buffer too small");
        for (int64_t off = 0; off < total; off += piece) {
            const int64_t cnt = std::min(piece, total - off);
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_comm, table + off, 8 * (size_t)cnt, hipMemcpyDeviceToDevice, ctx->stream));
            RSCHK(comm_allreduce_dev(ctx, 0, cnt, RSSEG_I64, RSSEG_SUM));
            HIPCHK(ctx, hipMemcpyAsync(table + off, ctx->d_comm, 8 * (size_t)cnt, hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    HIPCHK(ctx, hipMemcpyAsync(d_out, table, 8 * (size_t)cells, hipMemcpyDeviceToDevice, ctx->stream));
    unsigned long long h[2];
    RSCHK(kt_read(ctx, tail, sizeof(h), h));
    *n_left_out = (int64_t)h[0];
    if (h[1]) return rs_fail(ctx, RSSEG_ERR_INVALID, "class_moments: d_labels holds a counted label outside 0 ... %d", n_classes - 1);
    return RSSEG_OK;
}
