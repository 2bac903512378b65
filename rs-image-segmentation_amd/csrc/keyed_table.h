// The steps that the keyed-table kernels share (K23 segment sums, K24 class moments, K25 object table, K26 ISODATA sweep, K27
// region adjacency): pixels carry an integer key, integer terms are summed per key in a table in LDS, the table is added to a
// global table with 64-bit atomics, and a few counters come back through the pinned buffer.  Every step is defined once here
// (the wave scan, the fixed-point terms and the per-workgroup counter are in common.h); the kernels keep their own bodies.
#pragma once
#include <cmath>
#include <type_traits>

#include "common.h"

#define KT_TW 64         // tile columns: 16 threads x 4 pixels
#define KT_TH 16         // tile rows
#define KT_PXT 4         // consecutive pixels of one row per thread
#define KT_THREADS 256   // KT_TW * KT_TH / KT_PXT
#define KT_MAX_P 16      // planes of a raster call (K23, K25, K27)

struct kt_planes_t {
    const void *p[KT_MAX_P];
};

namespace {

// ---- host: argument checks.  Every text starts with the entry point's name `what`; an entry point calls them in the order in
// which it has always tested its arguments, which decides the refusal of a call with two faults.
inline int kt_check_hw(rsseg_ctx *ctx, const char *what, int H, int W)
{
    return H < 1 || W < 1 ? rs_fail(ctx, RSSEG_ERR_INVALID, "%s: H = %d, W = %d: both must be at least 1", what, H, W) : RSSEG_OK;
}
inline int kt_check_pixels(rsseg_ctx *ctx, const char *what, int64_t n)
{
    return n < 1 || n > 0x7fffffff ? rs_fail(ctx, RSSEG_ERR_INVALID, "%s: %lld pixels, must be 1 ... 2^31 - 1", what, (long long)n) : RSSEG_OK;
}
inline int kt_check_seg(rsseg_ctx *ctx, const char *what, const int32_t *d_seg)
{
    return !d_seg || ((uintptr_t)d_seg & 3) ? rs_fail(ctx, RSSEG_ERR_INVALID, "%s: d_seg null or not aligned to its element", what) : RSSEG_OK;
}
// max_text: how the bound is written (null: as a number)
inline int kt_check_nseg(rsseg_ctx *ctx, const char *what, int64_t n_segments, int64_t max_segments, const char *max_text)
{
    if (n_segments >= 0 && n_segments <= max_segments) return RSSEG_OK;
    if (max_text) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: n_segments = %lld is not in 0 ... %s", what, (long long)n_segments, max_text);
    return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: n_segments = %lld is not in 0 ... %lld", what, (long long)n_segments, (long long)max_segments);
}
// the segment raster of K25 / K27: a label is an int32; more rows than pixels are allowed (they stay empty)
inline int kt_check_raster(rsseg_ctx *ctx, const char *what, const int32_t *d_seg, int H, int W, int64_t n_segments)
{
    RSCHK(kt_check_hw(ctx, what, H, W));
    RSCHK(kt_check_pixels(ctx, what, (int64_t)H * W));
    RSCHK(kt_check_seg(ctx, what, d_seg));
    return kt_check_nseg(ctx, what, n_segments, 0x7fffffff, "2^31 - 1");
}
// the plane list of a raster call: min_p ... KT_MAX_P planes
inline int kt_check_planes(rsseg_ctx *ctx, const char *what, const void *d_planes, int P, int min_p)
{
    if (P < min_p || P > KT_MAX_P)
        return rs_fail(ctx, P < min_p ? RSSEG_ERR_INVALID : RSSEG_ERR_UNSUPPORTED, "%s: P = %d planes, must be %d ... %d", what, P, min_p, KT_MAX_P);
    if (P > 0 && !d_planes) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: d_planes is null", what);
    return RSSEG_OK;
}
// names: the two plane types in the words of the entry point's refusal
inline int kt_check_dtype(rsseg_ctx *ctx, const char *what, int dtype, const char *names)
{
    return dtype != RSSEG_U8 && dtype != RSSEG_F32 ? rs_fail(ctx, RSSEG_ERR_INVALID, "%s: dtype must be %s", what, names) : RSSEG_OK;
}
// one plane of uint8 or float32 elements
inline int kt_check_plane(rsseg_ctx *ctx, const char *what, const void *const *d_planes, int p, int dtype)
{
    if (!d_planes[p] || (dtype == RSSEG_F32 && ((uintptr_t)d_planes[p] & 3)))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: d_planes[%d] null or not aligned to its element", what, p);
    return RSSEG_OK;
}
inline int kt_check_plane_u8(rsseg_ctx *ctx, const char *what, const uint8_t *const *d_planes, int p)
{
    return !d_planes[p] ? rs_fail(ctx, RSSEG_ERR_INVALID, "%s: d_planes[%d] is null", what, p) : RSSEG_OK;
}
// the fixed point of K24 / K26: Q fraction bits, float32 planes scaled by 2^plane_exp[f], uint8 planes as they are
inline int kt_check_fixed(rsseg_ctx *ctx, const char *what, int dtype, const int *plane_exp, int Q, int64_t n_local)
{
    if (Q < 0 || Q > 50) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: Q=%d, must be 0 ... 50", what, Q);
    if (n_local >= ((int64_t)1 << (62 - Q))) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: n_local=%lld times 2^Q (Q=%d) reaches 2^62", what, (long long)n_local, Q);
    if (dtype == RSSEG_U8 && (plane_exp || Q != 0)) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: RSSEG_U8 planes take plane_exp = NULL and Q = 0", what);
    if (dtype == RSSEG_F32 && !plane_exp) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: plane_exp is null", what);
    return RSSEG_OK;
}
// *scale = 2^plane_exp[f] (1 without exponents)
inline int kt_plane_scale(rsseg_ctx *ctx, const char *what, const int *plane_exp, int f, double *scale)
{
    if (plane_exp && (plane_exp[f] < -300 || plane_exp[f] > 300))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: plane_exp[%d]=%d, must be -300 ... 300", what, f, plane_exp[f]);
    *scale = plane_exp ? std::ldexp(1.0, plane_exp[f]) : 1.0;
    return RSSEG_OK;
}

// ---- host: the tail.  Copies `bytes` at d_src to `out` through the pinned buffer and waits.
inline int kt_read(rsseg_ctx *ctx, const void *d_src, size_t bytes, void *out)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    memcpy(out, ctx->h_pin, bytes);
    return RSSEG_OK;
}
inline int kt_bad_labels(rsseg_ctx *ctx, const char *what, unsigned long long bad, int64_t n_segments)
{
    return bad ? rs_fail(ctx, RSSEG_ERR_INVALID, "%s: d_seg holds %llu labels outside 0 ... n_segments = %lld", what, bad, (long long)n_segments) : RSSEG_OK;
}

// ---- host: one launch on the context's stream; a kernel with dynamic LDS gets its limit raised first
template <typename... KA, typename... A>
int kt_launch(rsseg_ctx *ctx, void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, A... args)
{
    if (lds) RSCHK(set_max_dyn_lds(ctx, (const void *)kernel, lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, static_cast<KA>(args)...);
    return RSSEG_OK;
}

// ---- host: whether a thread's four pixels are one aligned word: every row starts aligned (W % 4 == 0) and so does every
// plane (align_mask: 3 for uint8, 15 for float32)
inline int kt_vec(int W, const void *const *d_planes, int P, uintptr_t align_mask)
{
    int vec = W % KT_PXT == 0;
    for (int p = 0; p < P; p++)
        if ((uintptr_t)d_planes[p] & align_mask) vec = 0;
    return vec;
}

}  // namespace

#ifdef __HIPCC__
// ---- device ------------------------------------------------------------------------------------------------------------
// the row of the tile and the first of the four columns of a thread
__device__ __forceinline__ int kt_ry(int tid) { return tid / (KT_TW / KT_PXT); }
__device__ __forceinline__ int kt_cx(int tid) { return (tid % (KT_TW / KT_PXT)) * KT_PXT; }

// An entry of a tile's list sorted by label (the counting sort of K24 step 2 and K26 step 3): label << 16 | slot
__device__ __forceinline__ uint32_t kt_sorted_entry(int label, int slot) { return ((uint32_t)label << 16) | (uint32_t)slot; }
__device__ __forceinline__ int kt_entry_label(uint32_t e) { return (int)(e >> 16); }
__device__ __forceinline__ int kt_entry_slot(uint32_t e) { return (int)(e & 0xffffu); }

// Path A: the workgroup's table in LDS, zeroed when the workgroup starts and added to the global table once, when it ends
// (non-zero cells only).  The caller puts a barrier behind the first and before the second.
template <int THREADS>
__device__ __forceinline__ void kt_table_zero(unsigned long long *l_table, int cells)
{
    for (int i = threadIdx.x; i < cells; i += THREADS) l_table[i] = 0;
}
template <int THREADS>
__device__ __forceinline__ void kt_table_flush(const unsigned long long *l_table, unsigned long long *__restrict__ g_table, int cells)
{
    for (int i = threadIdx.x; i < cells; i += THREADS) {
        const unsigned long long v = l_table[i];
        if (v) atomicAdd(&g_table[i], v);
    }
}
#endif
