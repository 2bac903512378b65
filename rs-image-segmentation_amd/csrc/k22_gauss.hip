// K22 — rsseg_gauss_classify: Gaussian maximum-likelihood / Mahalanobis / minimum-distance classification of feature-planar
// rasters.  One per-pixel sweep: per class a whitened quadratic form, then an arg-min with (on request) the runner-up.
// The arithmetic is the restatement's (tests/gaussian_ref.py), operation for operation, in float64:
//   x_f  = the plane value widened (exact), a NaN read as 0
//   d_f  = x_f - mean[j][f]
//   z_i  = fma chain over f = 0..i of W_j[i][f] * d_f, from +0        (W_j lower triangular, rows packed)
//   m_j  = fma chain over i = 0..F-1 of z_i * z_i, from +0
//   g_j  = m_j + offset[j];  j ascending: g_j < best -> (second, best, winner) = (best, g_j, j), else g_j < second -> second = g_j
// fma() stands where the restatement has one and nowhere else (the file is built with -ffp-contract=off like the rest).
//
// Registers.  A lane keeps its pixels' x in the planes' type for the whole class loop (FR planes x PXL pixels, PXL = one
// 16-byte load) and evaluates G (gc_shape: two, or all four at FR = 24) pixels at a time: d[.][G] in float64, every z_i folded into m as soon as its row ends.
// FR (compile time: 4, 8, 16, 24, 32, 64) is the smallest width that holds F; rows and columns at or beyond F are skipped by
// uniform branches.  Up to FR = 32 all of d is live (RB = FR).  The 64-wide form is blocked in the same operation order: rows
// in two blocks of RB = 32 whose z_i stay open while the columns go by in blocks of 32 (d of one column block live at a time,
// recomputed from x), so every z_i still sums f ascending and m still sums i ascending.  That form takes ONE pixel per lane
// with element loads (x[64] + z[32] + d[32] in float64 leave no room for a second): at F > 32 a pixel costs 64 times more
// float64 operations than bytes, so the width of its loads is not what the time goes to.
// Model parameters are read through uniform indices (the class loop and every unrolled row / column index are wave-uniform):
// scalar loads from the model's copy in the workspace, no per-lane gather.  The winner is carried as its class VALUE (a
// uniform scalar per class, 0 while nothing has won: class values are 1..255), so the label needs no table look-up either.
// MODE (compile time): GC_DIST writes float32(m_winner), GC_MARGIN carries the runner-up and writes float32(second - best);
// MODE 0 carries neither second nor the stores.  m of the winner is always carried (two registers per pixel): the threshold
// needs it.
#include <cmath>
#include <type_traits>

#include "common.h"

#define GC_THREADS 256
#define GC_DIST 1
#define GC_MARGIN 2
#define GC_G 2   // pixels evaluated together by one lane

struct gc_planes_t {
    const void *p[RSSEG_MAX_FEATURES];
};
struct gc_model_t {
    const double *mean;     // [k][F]
    const double *whiten;   // [k][F (F + 1) / 2]
    const double *offset;   // [k]
    const int *value;       // [k] class values, 1..255
};

template <typename T, int FR> struct gc_shape {
    static constexpr int PXL = FR > 32 ? 1 : 16 / (int)sizeof(T);   // pixels per lane and tile
    // pixels a lane evaluates together: every scalar-loaded parameter feeds G fma chains.  Two, which leaves the narrow forms
    // two to eight waves per SIMD; at FR = 24 two pixels already take the registers of half a SIMD, so that form evaluates all
    // PXL at once (x and d together: 12 FR registers for float32 planes) and halves its scalar loads at the same occupancy
    static constexpr int G = PXL < GC_G ? PXL : FR == 24 ? PXL : GC_G;
    static constexpr int RB = FR > 32 ? 32 : FR;                    // rows whose z stay open together; columns per d block
};

// the whitened quadratic form of G of the lane's pixels (p0 .. p0 + G - 1) for one class
template <typename T, int FR, int PXL, int G, int RB>
__device__ __forceinline__ void gc_form(const T (&x)[FR][PXL], int p0, int F, const double *__restrict__ mu, const double *__restrict__ w,
                                        double (&m)[G])
{
#pragma unroll
    for (int g = 0; g < G; g++) m[g] = 0.0;
#pragma unroll
    for (int rb = 0; rb < FR; rb += RB) {
        if (rb < F) {
            double z[RB][G];
#pragma unroll
            for (int r = 0; r < RB; r++)
#pragma unroll
                for (int g = 0; g < G; g++) z[r][g] = 0.0;
#pragma unroll
            for (int cb = 0; cb <= rb; cb += RB) {
                double d[RB][G];
#pragma unroll
                for (int c = 0; c < RB; c++) {
                    if (cb + c < F) {
                        const double mf = mu[cb + c];
#pragma unroll
                        for (int g = 0; g < G; g++) d[c][g] = (double)x[cb + c][p0 + g] - mf;
                    } else {
#pragma unroll
                        for (int g = 0; g < G; g++) d[c][g] = 0.0;
                    }
                }
#pragma unroll
                for (int r = 0; r < RB; r++) {
                    const int i = rb + r;
                    if (i < F) {
                        const double *__restrict__ wrow = w + (i * (i + 1)) / 2 + cb;
#pragma unroll
                        for (int c = 0; c < RB; c++) {
                            if (cb + c <= i) {   // compile time
                                const double wv = wrow[c];
#pragma unroll
                                for (int g = 0; g < G; g++) z[r][g] = fma(wv, d[c][g], z[r][g]);
                            }
                        }
                        if (cb == rb) {   // the row is complete: fold it into m, i ascending
#pragma unroll
                            for (int g = 0; g < G; g++) m[g] = fma(z[r][g], z[r][g], m[g]);
                        }
                    }
                }
            }
        }
    }
}

template <typename T, int FR, int MODE>
__global__ __launch_bounds__(GC_THREADS) void gauss_classify(gc_planes_t pl, int F, int k, int64_t n, gc_model_t md, double max_dist2, int vec,
                                                             uint8_t *__restrict__ labels, float *__restrict__ dist2, float *__restrict__ margin)
{
    constexpr int PXL = gc_shape<T, FR>::PXL, G = gc_shape<T, FR>::G, RB = gc_shape<T, FR>::RB;
    constexpr bool DIST = (MODE & GC_DIST) != 0, MARGIN = (MODE & GC_MARGIN) != 0;
    const int64_t base = ((int64_t)blockIdx.x * GC_THREADS + threadIdx.x) * PXL;
    if (base >= n) return;
    const bool whole = base + PXL <= n;
    T x[FR][PXL];
#pragma unroll
    for (int f = 0; f < FR; f++) {
        if (f < F) {
            const T *__restrict__ src = reinterpret_cast<const T *>(pl.p[f]);
            bool wide = false;
            if constexpr (PXL > 1) {   // PXL elements are 16 bytes
                wide = whole && (vec & 1);
                if (wide) {
                    const uint4 raw = *reinterpret_cast<const uint4 *>(src + base);
                    memcpy(x[f], &raw, 16);
                }
            }
            if (!wide) {
#pragma unroll
                for (int p = 0; p < PXL; p++) x[f][p] = base + p < n ? src[base + p] : (T)0;
            }
#pragma unroll
            for (int p = 0; p < PXL; p++)
                if (x[f][p] != x[f][p]) x[f][p] = (T)0;
        } else {
#pragma unroll
            for (int p = 0; p < PXL; p++) x[f][p] = (T)0;
        }
    }
    uint8_t lab[PXL];
    float dv[PXL], mv[PXL];
#pragma unroll
    for (int p0 = 0; p0 < PXL; p0 += G) {
        double best[G], second[G], bm[G];
        int win[G];   // the winner's class value; 0: none yet
#pragma unroll
        for (int g = 0; g < G; g++) {
            best[g] = second[g] = (double)INFINITY;
            bm[g] = 0.0;
            win[g] = 0;
        }
        const int tri = (F * (F + 1)) / 2;
        for (int j = 0; j < k; j++) {
            double m[G];
            gc_form<T, FR, PXL, G, RB>(x, p0, F, md.mean + (size_t)j * F, md.whiten + (size_t)j * tri, m);
            const double off = md.offset[j];
            const int cv = md.value[j];
#pragma unroll
            for (int g = 0; g < G; g++) {
                const double gj = m[g] + off;
                if (gj < best[g]) {
                    if constexpr (MARGIN) second[g] = best[g];
                    best[g] = gj;
                    bm[g] = m[g];
                    win[g] = cv;
                } else if constexpr (MARGIN) {
                    if (gj < second[g]) second[g] = gj;
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            const bool none = win[g] == 0;
            lab[p0 + g] = (uint8_t)((none || bm[g] > max_dist2) ? 0 : win[g]);
            if constexpr (DIST) dv[p0 + g] = none ? __uint_as_float(0x7fc00000u) : (float)bm[g];
            if constexpr (MARGIN) mv[p0 + g] = none ? __uint_as_float(0x7fc00000u) : (float)(second[g] - best[g]);
        }
    }
    // labels: PXL bytes in one store where the label plane is aligned to them
    if (PXL > 1 && whole && (vec & 2)) {
        if constexpr (PXL == 4) {
            uint32_t v;
            memcpy(&v, lab, 4);
            *reinterpret_cast<uint32_t *>(labels + base) = v;
        } else if constexpr (PXL == 2) {
            uint16_t v;
            memcpy(&v, lab, 2);
            *reinterpret_cast<uint16_t *>(labels + base) = v;
        }
    } else {
#pragma unroll
        for (int p = 0; p < PXL; p++)
            if (base + p < n) labels[base + p] = lab[p];
    }
    auto store_f = [&](float *__restrict__ out, const float (&v)[PXL], bool aligned) {
        if (PXL > 1 && whole && aligned) {
            if constexpr (PXL == 4) *reinterpret_cast<float4 *>(out + base) = make_float4(v[0], v[1], v[2], v[3]);
            else if constexpr (PXL == 2) *reinterpret_cast<float2 *>(out + base) = make_float2(v[0], v[1]);
        } else {
#pragma unroll
            for (int p = 0; p < PXL; p++)
                if (base + p < n) out[base + p] = v[p];
        }
    };
    if constexpr (DIST) store_f(dist2, dv, (vec & 4) != 0);
    if constexpr (MARGIN) store_f(margin, mv, (vec & 8) != 0);
}

namespace {

template <int V> using gc_ic = std::integral_constant<int, V>;

constexpr int gc_width(int F) { return F <= 4 ? 4 : F <= 8 ? 8 : F <= 16 ? 16 : F <= 24 ? 24 : F <= 32 ? 32 : 64; }

template <typename T, int FR>
int gc_launch_mode(rsseg_ctx *ctx, int mode, gc_planes_t pl, int F, int k, int64_t n, gc_model_t md, double max_dist2, uintptr_t planes_or,
                   uint8_t *labels, float *dist2, float *margin)
{
    constexpr int PXL = gc_shape<T, FR>::PXL;
    const int64_t blocks = ceil_div64(n, (int64_t)GC_THREADS * PXL);
    if (blocks > 0x7fffffff) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "gauss_classify: n=%lld pixels need more than 2^31 - 1 workgroups", (long long)n);
    // which accesses may be PXL elements wide: planes (16 bytes), labels (PXL bytes), dist2 / margin (4 PXL bytes)
    const int vec = ((planes_or & 15) == 0 ? 1 : 0) | (((uintptr_t)labels & (PXL - 1)) == 0 ? 2 : 0) |
                    (((uintptr_t)dist2 & (4 * PXL - 1)) == 0 ? 4 : 0) | (((uintptr_t)margin & (4 * PXL - 1)) == 0 ? 8 : 0);
    const dim3 grid((unsigned)blocks), block(GC_THREADS);
    auto go = [&](auto mode_c) {
        constexpr int MODE = decltype(mode_c)::value;
        hipLaunchKernelGGL((gauss_classify<T, FR, MODE>), grid, block, 0, ctx->stream, pl, F, k, n, md, max_dist2, vec, labels, dist2, margin);
    };
    switch (mode) {
    case 0: go(gc_ic<0>()); break;
    case GC_DIST: go(gc_ic<GC_DIST>()); break;
    case GC_MARGIN: go(gc_ic<GC_MARGIN>()); break;
    default: go(gc_ic<GC_DIST | GC_MARGIN>()); break;
    }
    return RSSEG_OK;
}

template <typename T, typename... A> int gc_launch(rsseg_ctx *ctx, int F, A... a)
{
    switch (gc_width(F)) {
    case 4: return gc_launch_mode<T, 4>(ctx, a...);
    case 8: return gc_launch_mode<T, 8>(ctx, a...);
    case 16: return gc_launch_mode<T, 16>(ctx, a...);
    case 24: return gc_launch_mode<T, 24>(ctx, a...);
    case 32: return gc_launch_mode<T, 32>(ctx, a...);
    default: return gc_launch_mode<T, 64>(ctx, a...);
    }
}

}  // namespace

extern "C" int rsseg_gauss_classify(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n, int k, const double *mean,
                                    const double *whiten, const double *offset, const uint8_t *class_values, double max_dist2, uint8_t *d_labels,
                                    float *d_dist2, float *d_margin)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || F < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: d_planes is empty (F=%d)", F);
    if (k < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: k=%d classes, must be >= 1", k);
    if (F > RSSEG_MAX_FEATURES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "gauss_classify: F=%d feature planes, the kernels take at most %d", F, RSSEG_MAX_FEATURES);
    if (k > RSSEG_MAX_CLUSTERS) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "gauss_classify: k=%d classes, the kernels take at most %d", k, RSSEG_MAX_CLUSTERS);
    if (dtype != RSSEG_F32 && dtype != RSSEG_F64) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: dtype must be RSSEG_F32 or RSSEG_F64");
    if (n < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: n=%lld is negative", (long long)n);
    if (!mean || !whiten || !offset || !class_values)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: the model (mean, whiten, offset, class_values) is missing");
    const int tri = F * (F + 1) / 2;
    auto finite = [&](const char *what, const double *v, int count) -> int {
        for (int i = 0; i < count; i++)
            if (!std::isfinite(v[i])) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: %s[%d] is not finite", what, i);
        return RSSEG_OK;
    };
    RSCHK(finite("mean", mean, k * F));
    RSCHK(finite("whiten", whiten, k * tri));
    RSCHK(finite("offset", offset, k));
    bool seen[256] = {false};
    for (int j = 0; j < k; j++) {
        if (class_values[j] == 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: class_values[%d] is 0, the value of an unclassified pixel", j);
        if (seen[class_values[j]]) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: class_values[%d]=%d occurs twice", j, (int)class_values[j]);
        seen[class_values[j]] = true;
    }
    if (max_dist2 != max_dist2) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: max_dist2 is NaN");
    if (n == 0) return RSSEG_OK;
    const size_t eb = dtype == RSSEG_F32 ? 4 : 8;
    gc_planes_t pl;
    memset(&pl, 0, sizeof(pl));
    uintptr_t planes_or = 0;
    for (int f = 0; f < F; f++) {
        if (!d_planes[f]) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: d_planes[%d] is null", f);
        if ((uintptr_t)d_planes[f] & (eb - 1)) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: d_planes[%d] is not aligned to its element", f);
        pl.p[f] = d_planes[f];
        planes_or |= (uintptr_t)d_planes[f];
    }
    if (!d_labels) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: d_labels is null");
    if ((uintptr_t)d_dist2 & 3) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: d_dist2 is not aligned to its element");
    if ((uintptr_t)d_margin & 3) return rs_fail(ctx, RSSEG_ERR_INVALID, "gauss_classify: d_margin is not aligned to its element");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the model as the kernel reads it, uploaded in one copy: mean, whiten, offset (float64), then the class values as ints
    const size_t n_mean = (size_t)k * F, n_wh = (size_t)k * tri;
    const size_t bytes = sizeof(double) * (n_mean + n_wh + (size_t)k) + sizeof(int) * (size_t)k;
    RSCHK(ws_reserve(ctx, bytes));
    RSCHK(pin_reserve(ctx, bytes));
    double *h = reinterpret_cast<double *>(ctx->h_pin);
    memcpy(h, mean, sizeof(double) * n_mean);
    memcpy(h + n_mean, whiten, sizeof(double) * n_wh);
    memcpy(h + n_mean + n_wh, offset, sizeof(double) * (size_t)k);
    int *hv = reinterpret_cast<int *>(h + n_mean + n_wh + k);
    for (int j = 0; j < k; j++) hv[j] = class_values[j];
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_ws, ctx->h_pin, bytes, hipMemcpyHostToDevice, ctx->stream));
    const double *d = reinterpret_cast<const double *>(ctx->d_ws);
    gc_model_t md;
    md.mean = d;
    md.whiten = d + n_mean;
    md.offset = d + n_mean + n_wh;
    md.value = reinterpret_cast<const int *>(d + n_mean + n_wh + k);
    const int mode = (d_dist2 ? GC_DIST : 0) | (d_margin ? GC_MARGIN : 0);
    {
        prof_scope ps(ctx, "gauss_classify");
        if (dtype == RSSEG_F32) RSCHK(gc_launch<float>(ctx, F, mode, pl, F, k, n, md, max_dist2, planes_or, d_labels, d_dist2, d_margin));
        else RSCHK(gc_launch<double>(ctx, F, mode, pl, F, k, n, md, max_dist2, planes_or, d_labels, d_dist2, d_margin));
        HIPCHK(ctx, hipGetLastError());
    }
    // the upload has to have left the pinned area before the next call writes into it
    HIPCHK(ctx, rs_sync(ctx));
    return RSSEG_OK;
}
