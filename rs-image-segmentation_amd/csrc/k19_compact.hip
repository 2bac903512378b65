// K19 — order-preserving stream compaction: a valid mask over feature planes, the planes compacted to their valid pixels in
// raster order, and per-pixel results expanded back to the raster with a fill value.  It lets the classifiers (K9, K11, K18)
// run unchanged on X[valid], exactly the matrix scikit-learn sees for a scene with a nodata collar and holes.
//
//   rsseg_valid_mask      one pass over P planes -> uint8 mask, valid count (one integer atomic per workgroup)
//   rsseg_compact_plan    count (one workgroup per tile) -> scan (ONE workgroup walks the tile counts) -> tile offsets
//   rsseg_compact_planes  out[p][rank(i)] = in[p][i] for valid i, all P planes in one launch
//   rsseg_expand_plane    out[i] = mask[i] ? in[rank(i)] : fill
//
// A TILE is K19_TILE = 4096 pixels = 256 threads x 16 mask bytes (one 16-byte load per thread where the mask is 16-byte aligned).
// Thread t owns the pixels [16 t, 16 t + 16) of its tile: a 16-bit map of their non-zero mask bytes and, from a wave prefix
// (__shfl_up over 64 lanes) plus the four wave totals in LDS, the rank of its first pixel within the tile.  Map and rank go
// into a 1 KiB LDS table once per tile and are reused by every plane.
// The planes are walked in 16-byte vectors, lane-contiguous (thread t of pass q has the vector (256 q + t)): a vector lies
// inside ONE owner's 16 pixels, so its elements' ranks are the owner's rank plus a popcount of the map below the vector.
// Compaction stages a tile's survivors in LDS at the index their global destination has modulo 16 bytes, so that the copy out
// is 16-byte stores wherever a whole vector of the destination belongs to the tile and element stores at its two ragged ends
// (a vector is never shared between two tiles' vector stores: each tile stores only the elements it owns).  Measured on 15
// float32 planes at 16384 x 16384 (profiles/compact_bench.json) the staged store takes 0.61 - 0.84 of the time of storing the
// survivors element by element straight to global memory (K19_STAGED_STORE = 0), so it stays.
// Expansion fetches each lane's survivors straight from the compacted plane (consecutive elements from the tile's offset plus
// the rank) and writes whole 16-byte vectors of the raster.  Staging the tile's compacted run through LDS the same way
// (K19_STAGED_FETCH = 1) measured within 3 % either way, so the simpler form is the one built.
// No workgroup waits for another: the scan over tile totals is a launch of its own, count -> scan -> consume.
// LDS: compaction's staging buffer (K19_TILE elements + one vector), the 1 KiB owner table and four wave totals.  No scratch.
#include <algorithm>

#include "common.h"

// the two alternatives profiles/compact_bench.py measures against the forms above (a second build of the library)
#ifndef K19_STAGED_STORE
#define K19_STAGED_STORE 1
#endif
#ifndef K19_STAGED_FETCH
#define K19_STAGED_FETCH 0
#endif

#define K19_THREADS 256
#define K19_PXT 16                          // mask bytes per thread
#define K19_TILE (K19_THREADS * K19_PXT)    // 4096 pixels
#define K19_SCAN_ITEMS 4
#define K19_SCAN_SPAN (K19_THREADS * K19_SCAN_ITEMS)   // tiles per pass of the scan workgroup
#define K19_MAX_N ((int64_t)1 << 39)         // every grid stays below 2^31 workgroups
#define K19_MAX_PLANES 64                   // per launch; longer lists go in several launches

extern "C" int rsseg_compact_tile(void) { return K19_TILE; }
extern "C" int rsseg_compact_scan_span(void) { return K19_SCAN_SPAN; }

struct k19_planes_t {
    const void *in[K19_MAX_PLANES];
    void *out[K19_MAX_PLANES];
};
struct k19_src_t {
    const void *p[K19_MAX_PLANES];
};

// ---- per-tile owner record -------------------------------------------------------------------------------------
// the 16-bit map of thread t's non-zero mask bytes (bit j: pixel tile0 + 16 t + j); pixels at or beyond n read as 0
__device__ __forceinline__ unsigned k19_map(const uint8_t *__restrict__ mask, int64_t tile0, int64_t n, bool vec)
{
    const int64_t base = tile0 + (int64_t)threadIdx.x * K19_PXT;
    unsigned m = 0;
    if (vec && base + K19_PXT <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(mask + base);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < K19_PXT; j++) m |= (((w[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0u ? 1u : 0u) << j;
    } else {
#pragma unroll
        for (int j = 0; j < K19_PXT; j++)
            if (base + j < n) m |= (mask[base + j] != 0 ? 1u : 0u) << j;
    }
    return m;
}

// exclusive prefix of `c` over the workgroup's 256 threads; *total = the workgroup's sum.  s_w: 4 ints of LDS.  All threads.
__device__ __forceinline__ int k19_wg_prefix(int c, int *s_w, int *total)
{
    int incl = c;   // wave_incl_scan written out: the helper reorders k19_scan
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane_id() >= o) incl += up;
    }
    const int w = threadIdx.x >> 6;
    if (lane_id() == 63) s_w[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int t = s_w[i];
        if (i < w) before += t;
        all += t;
    }
    *total = all;
    return before + incl - c;
}

// fills s_own[t] = map | rank << 16 for the tile; ends with a barrier.  Returns the tile's valid count.
__device__ __forceinline__ int k19_owner_table(const uint8_t *__restrict__ mask, int64_t tile0, int64_t n, bool vec, unsigned *s_own, int *s_w)
{
    const unsigned m = k19_map(mask, tile0, n, vec);
    int total;
    const int rank = k19_wg_prefix(__popc(m), s_w, &total);
    s_own[threadIdx.x] = m | ((unsigned)rank << 16);   // rank <= 4096 - 1 when the map is non-empty; 4096 fits 16 bits too
    __syncthreads();
    return total;
}

// ---- count and scan ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(K19_THREADS) void k19_count(const uint8_t *__restrict__ mask, int64_t n, int vec, int64_t *__restrict__ off)
{
    __shared__ int s_w[4];
    const int64_t tile0 = (int64_t)blockIdx.x * K19_TILE;
    const unsigned m = k19_map(mask, tile0, n, vec != 0);
    int total;
    k19_wg_prefix(__popc(m), s_w, &total);
    if (threadIdx.x == 0) off[blockIdx.x] = total;
}

// one workgroup: off[0 .. ntiles) counts -> exclusive prefix in place, off[ntiles] = the sum
__global__ __launch_bounds__(K19_THREADS) void k19_scan(int64_t *__restrict__ off, int64_t ntiles)
{
    __shared__ int s_w[4];
    int64_t carry = 0;
    for (int64_t base = 0; base < ntiles; base += K19_SCAN_SPAN) {
        const int64_t i0 = base + (int64_t)threadIdx.x * K19_SCAN_ITEMS;
        int v[K19_SCAN_ITEMS], c = 0;
#pragma unroll
        for (int j = 0; j < K19_SCAN_ITEMS; j++) {
            v[j] = i0 + j < ntiles ? (int)off[i0 + j] : 0;   // a count is at most K19_TILE; a pass sums to at most 2^22
            c += v[j];
        }
        int total;
        int64_t run = carry + k19_wg_prefix(c, s_w, &total);
#pragma unroll
        for (int j = 0; j < K19_SCAN_ITEMS; j++) {
            if (i0 + j < ntiles) off[i0 + j] = run;
            run += v[j];
        }
        carry += total;
        __syncthreads();   // s_w is rewritten by the next pass
    }
    if (threadIdx.x == 0) off[ntiles] = carry;
}

// ---- compaction ---------------------------------------------------------------------------------------------------
template <int E> struct k19_elem;
template <> struct k19_elem<1> { typedef uint8_t type; };
template <> struct k19_elem<4> { typedef uint32_t type; };
template <> struct k19_elem<8> { typedef uint64_t type; };

template <int E>
__global__ __launch_bounds__(K19_THREADS) void k19_compact(const uint8_t *__restrict__ mask, int mask_vec, const int64_t *__restrict__ off, int64_t n,
                                                           k19_planes_t pl, int P)
{
    typedef typename k19_elem<E>::type T;
    constexpr int VEC = 16 / E;                 // elements per 16-byte vector
    constexpr int PASSES = K19_TILE / (K19_THREADS * VEC);
    __shared__ unsigned s_own[K19_THREADS];
    __shared__ int s_w[4];
#if K19_STAGED_STORE
    __shared__ __align__(16) T s_stage[K19_TILE + VEC];
#endif
    const int64_t tile0 = (int64_t)blockIdx.x * K19_TILE;
    const int cnt = k19_owner_table(mask, tile0, n, mask_vec != 0, s_own, s_w);
    if (cnt == 0) return;   // uniform
    const int64_t dst0 = off[blockIdx.x];
    const bool full = tile0 + K19_TILE <= n;
    for (int p = 0; p < P; p++) {
        const T *__restrict__ in = reinterpret_cast<const T *>(pl.in[p]);
        T *__restrict__ out = reinterpret_cast<T *>(pl.out[p]);
        const bool in_vec = full && ((uintptr_t)in & 15) == 0;
#if K19_STAGED_STORE
        const int shift = (int)(((uintptr_t)(out + dst0) / E) & (VEC - 1));
        T *dst = s_stage + shift;
#else
        T *dst = out + dst0;
#endif
#pragma unroll
        for (int q = 0; q < PASSES; q++) {
            const int e0 = (q * K19_THREADS + threadIdx.x) * VEC;   // first pixel of this thread's vector, tile-relative
            const unsigned own = s_own[e0 / K19_PXT];
            const int sub = e0 % K19_PXT;
            const unsigned bits = ((own & 0xffffu) >> sub) & ((1u << VEC) - 1u);
            if (bits == 0) continue;
            int r = (int)(own >> 16) + __popc(own & ((1u << sub) - 1u));
            T v[VEC];
            if (in_vec) {
                const uint4 raw = *reinterpret_cast<const uint4 *>(in + tile0 + e0);
                memcpy(v, &raw, 16);
            } else {
#pragma unroll
                for (int j = 0; j < VEC; j++) v[j] = (bits >> j) & 1u ? in[tile0 + e0 + j] : (T)0;   // a set bit is a pixel below n
            }
#pragma unroll
            for (int j = 0; j < VEC; j++)
                if ((bits >> j) & 1u) dst[r++] = v[j];
        }
#if K19_STAGED_STORE
        __syncthreads();
        // copy out: vector v of the staging buffer is the 16 aligned bytes at (out + dst0 - shift) + v * VEC
        T *gbase = out + dst0 - shift;
        const int lo = shift, hi = shift + cnt;   // staged elements [lo, hi)
        for (int v0 = threadIdx.x * VEC; v0 < hi; v0 += K19_THREADS * VEC) {
            if (v0 >= lo && v0 + VEC <= hi) {
                *reinterpret_cast<uint4 *>(gbase + v0) = *reinterpret_cast<const uint4 *>(s_stage + v0);
            } else {
#pragma unroll
                for (int j = 0; j < VEC; j++)
                    if (v0 + j >= lo && v0 + j < hi) gbase[v0 + j] = s_stage[v0 + j];
            }
        }
        __syncthreads();   // the next plane rewrites the staging buffer
#endif
    }
}

// ---- expansion ----------------------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(K19_THREADS) void k19_expand(const uint8_t *__restrict__ mask, int mask_vec, const int64_t *__restrict__ off, int64_t n,
                                                          const typename k19_elem<E>::type *__restrict__ in, typename k19_elem<E>::type fill,
                                                          typename k19_elem<E>::type *__restrict__ out)
{
    typedef typename k19_elem<E>::type T;
    constexpr int VEC = 16 / E;
    constexpr int PASSES = K19_TILE / (K19_THREADS * VEC);
    __shared__ unsigned s_own[K19_THREADS];
    __shared__ int s_w[4];
    const int64_t tile0 = (int64_t)blockIdx.x * K19_TILE;
    const int cnt = k19_owner_table(mask, tile0, n, mask_vec != 0, s_own, s_w);
    const int64_t src0 = off[blockIdx.x];
#if K19_STAGED_FETCH
    __shared__ __align__(16) T s_stage[K19_TILE + VEC];
    const int shift = (int)(((uintptr_t)(in + src0) / E) & (VEC - 1));
    {
        const T *gbase = in + src0 - shift;
        const int lo = shift, hi = shift + cnt;
        for (int v0 = threadIdx.x * VEC; v0 < hi; v0 += K19_THREADS * VEC) {
            if (v0 >= lo && v0 + VEC <= hi) {
                *reinterpret_cast<uint4 *>(s_stage + v0) = *reinterpret_cast<const uint4 *>(gbase + v0);
            } else {
#pragma unroll
                for (int j = 0; j < VEC; j++)
                    if (v0 + j >= lo && v0 + j < hi) s_stage[v0 + j] = gbase[v0 + j];
            }
        }
        __syncthreads();
    }
    const T *src = s_stage + shift;
#else
    const T *src = in + src0;
#endif
    const bool out_vec = tile0 + K19_TILE <= n && ((uintptr_t)out & 15) == 0;
#pragma unroll
    for (int q = 0; q < PASSES; q++) {
        const int e0 = (q * K19_THREADS + threadIdx.x) * VEC;
        if (tile0 + e0 >= n) continue;
        const unsigned own = s_own[e0 / K19_PXT];
        const int sub = e0 % K19_PXT;
        const unsigned bits = ((own & 0xffffu) >> sub) & ((1u << VEC) - 1u);
        int r = (int)(own >> 16) + __popc(own & ((1u << sub) - 1u));
        T v[VEC];
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            v[j] = fill;
            if ((bits >> j) & 1u) v[j] = src[r++];
        }
        if (out_vec) {
            uint4 raw;
            memcpy(&raw, v, 16);
            *reinterpret_cast<uint4 *>(out + tile0 + e0) = raw;
        } else {
#pragma unroll
            for (int j = 0; j < VEC; j++)
                if (tile0 + e0 + j < n) out[tile0 + e0 + j] = v[j];
        }
    }
}

// ---- valid mask ---------------------------------------------------------------------------------------------------
template <typename T> struct k19_px;
template <> struct k19_px<float> { static constexpr int N = 4; typedef uint32_t store; };
template <> struct k19_px<double> { static constexpr int N = 2; typedef uint16_t store; };
template <> struct k19_px<uint8_t> { static constexpr int N = 16; typedef uint4 store; };

template <typename T> __device__ __forceinline__ bool k19_bad(T x, int flags, T nodata)
{
    bool bad = false;
    if constexpr (sizeof(T) > 1) {
        if (flags & RSSEG_VALID_NAN) bad = bad || x != x;
        if (flags & RSSEG_VALID_INF) bad = bad || x == (T)INFINITY || x == -(T)INFINITY;
    }
    if (flags & RSSEG_VALID_VALUE) bad = bad || x == nodata;
    return bad;
}

// one thread: N = 16 / sizeof(T) pixels of every plane (one 16-byte load per plane), N mask bytes
template <typename T>
__global__ __launch_bounds__(K19_THREADS) void k19_valid(k19_src_t pl, int P, int64_t n, int flags, T nodata, const uint8_t *__restrict__ d_and,
                                                         uint8_t *__restrict__ d_mask, int all_vec, int mask_vec, unsigned long long *__restrict__ count)
{
    constexpr int N = k19_px<T>::N;
    const int64_t base = ((int64_t)blockIdx.x * K19_THREADS + threadIdx.x) * N;
    unsigned bad = 0;   // bit j: pixel base + j is not valid
    const bool whole = base + N <= n;
    if (base < n) {
        for (int p = 0; p < P; p++) {
            const T *__restrict__ x = reinterpret_cast<const T *>(pl.p[p]);
            T v[N];
            if (whole && all_vec) {
                const uint4 raw = *reinterpret_cast<const uint4 *>(x + base);
                memcpy(v, &raw, 16);
            } else {
#pragma unroll
                for (int j = 0; j < N; j++) v[j] = base + j < n ? x[base + j] : (T)0;
            }
#pragma unroll
            for (int j = 0; j < N; j++) bad |= (k19_bad<T>(v[j], flags, nodata) ? 1u : 0u) << j;
        }
        if (d_and) {
#pragma unroll
            for (int j = 0; j < N; j++)
                if (base + j < n && d_and[base + j] == 0) bad |= 1u << j;
        }
    }
    int c = 0;
    if (whole && mask_vec) {   // N mask bytes in one store
        uint8_t ok[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
            ok[j] = (bad >> j) & 1u ? 0 : 1;
            c += ok[j];
        }
        typename k19_px<T>::store st;
        memcpy(&st, ok, N);
        *reinterpret_cast<typename k19_px<T>::store *>(d_mask + base) = st;
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) {
            if (base + j < n) {
                const uint8_t ok = (bad >> j) & 1u ? 0 : 1;
                d_mask[base + j] = ok;
                c += ok;
            }
        }
    }
    __shared__ int s_c[4];
    c = wave_sum(c);
    if (lane_id() == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = s_c[0] + s_c[1] + s_c[2] + s_c[3];
        if (t) atomicAdd(count, (unsigned long long)t);
    }
}

namespace {

int64_t k19_tiles(int64_t n) { return ceil_div64(n, K19_TILE); }

int k19_read_i64(rsseg_ctx *ctx, const void *d_src, int64_t *out)
{
    RSCHK(pin_reserve(ctx, sizeof(int64_t)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_src, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    memcpy(out, ctx->h_pin, sizeof(int64_t));
    return RSSEG_OK;
}

template <typename T>
int valid_launch(rsseg_ctx *ctx, const void *const *d_planes, int P, int64_t n, int flags, T nodata, const uint8_t *d_and, uint8_t *d_mask,
                 unsigned long long *d_count)
{
    constexpr int N = k19_px<T>::N;
    k19_src_t pl;
    memset(&pl, 0, sizeof(pl));
    int all_vec = 1;
    for (int p = 0; p < P; p++) {
        pl.p[p] = d_planes[p];
        if ((uintptr_t)d_planes[p] & 15) all_vec = 0;
    }
    const int64_t blocks = ceil_div64(n, (int64_t)K19_THREADS * N);
    hipLaunchKernelGGL(k19_valid<T>, dim3((unsigned)blocks), dim3(K19_THREADS), 0, ctx->stream, pl, P, n, flags, nodata, d_and, d_mask, all_vec,
                       ((uintptr_t)d_mask & 15) == 0 ? 1 : 0, d_count);
    return RSSEG_OK;
}

}  // namespace

extern "C" int rsseg_valid_mask(rsseg_ctx *ctx, const void *const *d_planes, int P, int dtype, int64_t n, int flags, double nodata,
                                const uint8_t *d_and, uint8_t *d_mask, int64_t *n_valid)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || P < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "valid_mask: d_planes is empty (P=%d)", P);
    if (P > K19_MAX_PLANES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "valid_mask: P=%d planes, one call takes at most %d", P, K19_MAX_PLANES);
    if (dtype != RSSEG_F32 && dtype != RSSEG_F64 && dtype != RSSEG_U8)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "valid_mask: dtype must be RSSEG_F32, RSSEG_F64 or RSSEG_U8");
    if (n < 0 || n >= K19_MAX_N) return rs_fail(ctx, RSSEG_ERR_INVALID, "valid_mask: n=%lld out of range", (long long)n);
    if (flags & ~(RSSEG_VALID_NAN | RSSEG_VALID_INF | RSSEG_VALID_VALUE)) return rs_fail(ctx, RSSEG_ERR_INVALID, "valid_mask: unknown bits in flags=%d", flags);
    if (!n_valid) return rs_fail(ctx, RSSEG_ERR_INVALID, "valid_mask: n_valid is null");
    *n_valid = 0;
    if (n == 0) return RSSEG_OK;
    if (!d_mask) return rs_fail(ctx, RSSEG_ERR_INVALID, "valid_mask: d_mask is null");
    const size_t eb = dtype == RSSEG_F32 ? 4 : dtype == RSSEG_F64 ? 8 : 1;
    for (int p = 0; p < P; p++)
        if (!d_planes[p] || ((uintptr_t)d_planes[p] & (eb - 1))) return rs_fail(ctx, RSSEG_ERR_INVALID, "valid_mask: d_planes[%d] null or not aligned to its element", p);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RSCHK(ws_reserve(ctx, 256));
    unsigned long long *d_count = reinterpret_cast<unsigned long long *>(ctx->d_ws);
    HIPCHK(ctx, hipMemsetAsync(d_count, 0, sizeof(*d_count), ctx->stream));
    {
        prof_scope ps(ctx, "valid_mask");
        if (dtype == RSSEG_F32) {
            RSCHK(valid_launch<float>(ctx, d_planes, P, n, flags, (float)nodata, d_and, d_mask, d_count));
        } else if (dtype == RSSEG_F64) {
            RSCHK(valid_launch<double>(ctx, d_planes, P, n, flags, nodata, d_and, d_mask, d_count));
        } else {
            // a value no byte holds matches nothing
            const bool byte = nodata >= 0.0 && nodata <= 255.0 && nodata == (double)(uint8_t)nodata;
            RSCHK(valid_launch<uint8_t>(ctx, d_planes, P, n, byte ? flags : (flags & ~RSSEG_VALID_VALUE), byte ? (uint8_t)nodata : (uint8_t)0, d_and,
                                        d_mask, d_count));
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return k19_read_i64(ctx, d_count, n_valid);
}

extern "C" int rsseg_compact_plan(rsseg_ctx *ctx, const uint8_t *d_mask, int64_t n, int64_t *d_tile_off, int64_t *n_valid)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (n < 0 || n >= K19_MAX_N) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_plan: n=%lld out of range", (long long)n);
    if (!d_tile_off || ((uintptr_t)d_tile_off & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_plan: d_tile_off null or not 8-byte aligned");
    if (n > 0 && !d_mask) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_plan: d_mask is null");
    if (!n_valid) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_plan: n_valid is null");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t ntiles = k19_tiles(n);
    if (ntiles == 0) {
        HIPCHK(ctx, hipMemsetAsync(d_tile_off, 0, sizeof(int64_t), ctx->stream));
    } else {
        prof_scope ps(ctx, "compact_plan");
        hipLaunchKernelGGL(k19_count, dim3((unsigned)ntiles), dim3(K19_THREADS), 0, ctx->stream, d_mask, n, ((uintptr_t)d_mask & 15) == 0 ? 1 : 0, d_tile_off);
        hipLaunchKernelGGL(k19_scan, dim3(1), dim3(K19_THREADS), 0, ctx->stream, d_tile_off, ntiles);
        HIPCHK(ctx, hipGetLastError());
    }
    return k19_read_i64(ctx, d_tile_off + ntiles, n_valid);
}

extern "C" int rsseg_compact_planes(rsseg_ctx *ctx, const uint8_t *d_mask, const int64_t *d_tile_off, int64_t n, const void *const *d_in, int P,
                                    int elem_bytes, void *const *d_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (n < 0 || n >= K19_MAX_N) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: n=%lld out of range", (long long)n);
    if (P < 0 || (P > 0 && (!d_in || !d_out))) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: d_in / d_out null (P=%d)", P);
    if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: elem_bytes=%d, must be 1, 4 or 8", elem_bytes);
    if (n == 0 || P == 0) return RSSEG_OK;
    if (!d_mask) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: d_mask is null");
    if (!d_tile_off || ((uintptr_t)d_tile_off & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: d_tile_off null or not 8-byte aligned");
    for (int p = 0; p < P; p++) {
        if (!d_in[p] || ((uintptr_t)d_in[p] & (elem_bytes - 1))) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: d_in[%d] null or not aligned to its element", p);
        if (!d_out[p] || ((uintptr_t)d_out[p] & (elem_bytes - 1))) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: d_out[%d] null or not aligned to its element", p);
        if (d_out[p] == d_in[p]) return rs_fail(ctx, RSSEG_ERR_INVALID, "compact_planes: d_out[%d] aliases d_in[%d]", p, p);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t ntiles = k19_tiles(n);
    const int mask_vec = ((uintptr_t)d_mask & 15) == 0 ? 1 : 0;
    {
        prof_scope ps(ctx, "compact");
        for (int p0 = 0; p0 < P; p0 += K19_MAX_PLANES) {
            const int np = std::min(P - p0, K19_MAX_PLANES);
            k19_planes_t pl;
            memset(&pl, 0, sizeof(pl));
            for (int p = 0; p < np; p++) {
                pl.in[p] = d_in[p0 + p];
                pl.out[p] = d_out[p0 + p];
            }
            const dim3 grid((unsigned)ntiles), block(K19_THREADS);
            if (elem_bytes == 1) hipLaunchKernelGGL(k19_compact<1>, grid, block, 0, ctx->stream, d_mask, mask_vec, d_tile_off, n, pl, np);
            else if (elem_bytes == 4) hipLaunchKernelGGL(k19_compact<4>, grid, block, 0, ctx->stream, d_mask, mask_vec, d_tile_off, n, pl, np);
            else hipLaunchKernelGGL(k19_compact<8>, grid, block, 0, ctx->stream, d_mask, mask_vec, d_tile_off, n, pl, np);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return stream_sync(ctx);
}

extern "C" int rsseg_expand_plane(rsseg_ctx *ctx, const uint8_t *d_mask, const int64_t *d_tile_off, int64_t n, const void *d_in, int elem_bytes,
                                  const void *fill, void *d_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (n < 0 || n >= K19_MAX_N) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: n=%lld out of range", (long long)n);
    if (elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: elem_bytes=%d, must be 1, 4 or 8", elem_bytes);
    if (!fill) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: fill is null");
    if (n == 0) return RSSEG_OK;
    if (!d_mask) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: d_mask is null");
    if (!d_tile_off || ((uintptr_t)d_tile_off & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: d_tile_off null or not 8-byte aligned");
    if (!d_out || ((uintptr_t)d_out & (elem_bytes - 1))) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: d_out null or not aligned to its element");
    if ((uintptr_t)d_in & (elem_bytes - 1)) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: d_in not aligned to its element");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t ntiles = k19_tiles(n);
    // d_in holds n_valid <= n elements (it may be null when there are none): an output that begins inside it is refused at once,
    // an input that begins below the output is measured against the plan's own count
    const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out, span = (uintptr_t)n * elem_bytes;
    if (d_in && a >= b && a < b + span) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: d_out aliases d_in");
    if (!d_in || (a < b && a + span > b)) {
        int64_t nv = 0;
        RSCHK(k19_read_i64(ctx, d_tile_off + ntiles, &nv));
        if (nv > 0 && !d_in) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: d_in is null");
        if (d_in && a + (uintptr_t)nv * elem_bytes > b) return rs_fail(ctx, RSSEG_ERR_INVALID, "expand_plane: d_out aliases d_in");
    }
    const int mask_vec = ((uintptr_t)d_mask & 15) == 0 ? 1 : 0;
    {
        prof_scope ps(ctx, "expand");
        const dim3 grid((unsigned)ntiles), block(K19_THREADS);
        if (elem_bytes == 1) {
            uint8_t f;
            memcpy(&f, fill, 1);
            hipLaunchKernelGGL(k19_expand<1>, grid, block, 0, ctx->stream, d_mask, mask_vec, d_tile_off, n, (const uint8_t *)d_in, f, (uint8_t *)d_out);
        } else if (elem_bytes == 4) {
            uint32_t f;
            memcpy(&f, fill, 4);
            hipLaunchKernelGGL(k19_expand<4>, grid, block, 0, ctx->stream, d_mask, mask_vec, d_tile_off, n, (const uint32_t *)d_in, f, (uint32_t *)d_out);
        } else {
            uint64_t f;
            memcpy(&f, fill, 8);
            hipLaunchKernelGGL(k19_expand<8>, grid, block, 0, ctx->stream, d_mask, mask_vec, d_tile_off, n, (const uint64_t *)d_in, f, (uint64_t *)d_out);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    return stream_sync(ctx);
}
