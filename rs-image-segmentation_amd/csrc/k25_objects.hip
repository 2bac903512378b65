// K25 — the object table: per segment the count, the coordinate moments, the bounding box, the perimeter and, per plane, the
// sum, the sum of squares, the minimum and the maximum (include/rsseg.h, rsseg_segment_features).  Everything is an integer
// sum, minimum or maximum, so the table has one right answer whatever the order the atomics land in; it is restated in NumPy
// in tests/objects_ref.py, to which the kernel is equal bit for bit.
//
// A workgroup walks the 64 x 16 tiles of keyed_table.h (grid stride); a thread owns four consecutive pixels of a row.
//   1. The EFFECTIVE labels of the tile and of a one-pixel ring around it are staged in LDS: the label where it is
//      1 ... n_segments and the mask byte is non-zero, else 0 (outside the image: 0).  A label outside 0 ... n_segments is
//      counted for the refusal and reads as 0, so it never becomes an index.
//   2. The segments met in the tile share a table of K25_SLOTS rows in LDS, found by open addressing on the label (linear
//      probing over the WHOLE table, so exactly K25_SLOTS different labels still fit).  A thread adds a RUN of equal labels at
//      once, with native 64-bit LDS adds / minima / maxima.  A label that finds no row commits its runs straight to the global
//      table.
//   3. Every occupied row is flushed once per tile with 64-bit global atomics, consecutive lanes on consecutive columns of a
//      row, and put back to the empty pattern as it is read; the LDS table is therefore initialised once per workgroup.
// Empty pattern of a column: 0 for a sum, INT64_MAX / INT64_MIN (H / -1, W / -1 for the bounding box) for a minimum / maximum.
#include <algorithm>

#include "keyed_table.h"

#define K25_SLOTS 64     // rows of the LDS table (a power of two); 64 x (11 + 4 * 16) x 8 B = 37.5 KiB at P = 16
#define K25_GEO 11       // geometry columns
#define K25_MAX_BLOCKS 8192
#define K25_EW (KT_TW + 2)
#define K25_EH (KT_TH + 2)
static_assert(K25_SLOTS == 64, "the hash keeps the top six bits of the product: change the shift with the row count");
static_assert(K25_SLOTS <= KT_THREADS && KT_TW * KT_TH == KT_THREADS * KT_PXT, "one thread per row of the list; four pixels per thread");

extern "C" void rsseg_segment_features_plan(int P, int *tile_w, int *tile_h, int *lds_slots)
{
    (void)P;   // the plan does not depend on the plane count: the row gets wider, the table keeps its rows
    if (tile_w) *tile_w = KT_TW;
    if (tile_h) *tile_h = KT_TH;
    if (lds_slots) *lds_slots = K25_SLOTS;
}

// what a column holds: 0 a sum, 1 a minimum, 2 a maximum
__host__ __device__ __forceinline__ int k25_kind(int col)
{
    if (col < K25_GEO) return col == 6 || col == 8 ? 1 : (col == 7 || col == 9 ? 2 : 0);
    const int f = (col - K25_GEO) & 3;
    return f == 2 ? 1 : (f == 3 ? 2 : 0);
}
__host__ __device__ __forceinline__ long long k25_empty(int col, int H, int W)
{
    if (col < K25_GEO) return col == 6 ? H : (col == 8 ? W : (col == 7 || col == 9 ? -1 : 0));
    const int f = (col - K25_GEO) & 3;
    return f == 2 ? INT64_MAX : (f == 3 ? INT64_MIN : 0);
}

// one value into one column of a table row, in LDS or in global memory (the address space follows the pointer)
__device__ __forceinline__ void k25_put(long long *cell, int kind, long long v)
{
    if (kind == 0) atomicAdd(reinterpret_cast<unsigned long long *>(cell), (unsigned long long)v);
    else if (kind == 1) atomicMin(cell, v);
    else atomicMax(cell, v);
}

// llrint(v * v * 2^24): the square of a float32 is exact in float64 and below 2^22, so the scaled value stays below 2^51
__device__ __forceinline__ long long k25_sq_fixed24(double v) { return fx_round(v * v, 16777216.0); }

__global__ __launch_bounds__(KT_THREADS) void k25_init(long long *__restrict__ table, int64_t rows, int C, int H, int W)
{
    const int64_t total = rows * C;
    for (int64_t e = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * KT_THREADS)
        table[e] = k25_empty((int)(e % C), H, W);
}

template <typename T, bool GEO>
__global__ __launch_bounds__(KT_THREADS) void k25_features(const int *__restrict__ seg, const uint8_t *__restrict__ mask, int H, int W, int64_t nseg,
                                                            kt_planes_t pl, int P, int vec, int tiles_x, int64_t ntiles, long long *__restrict__ table,
                                                            unsigned long long *__restrict__ bad)
{
    extern __shared__ __align__(8) unsigned char k25_lds[];
    __shared__ int s_eff[K25_EH][K25_EW];   // effective labels of the tile and its ring
    __shared__ int s_key[K25_SLOTS];        // 0: free, else the label the row belongs to
    __shared__ int s_list[K25_SLOTS];       // the occupied rows, in the order they were claimed
    __shared__ int s_nocc;
    long long *s_tab = reinterpret_cast<long long *>(k25_lds);   // [K25_SLOTS][C]
    const int C = K25_GEO + 4 * P, tid = threadIdx.x;
    for (int e = tid; e < K25_SLOTS * C; e += KT_THREADS) s_tab[e] = k25_empty(e % C, H, W);
    if (tid < K25_SLOTS) s_key[tid] = 0;
    if (tid == 0) s_nocc = 0;
    const int ry = kt_ry(tid), cx = kt_cx(tid);
    unsigned nbad = 0;

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx0 = (int)(t % tiles_x) * KT_TW, ty0 = (int)(t / tiles_x) * KT_TH;
        __syncthreads();   // the table is empty and the previous tile's labels are no longer read
        for (int e = tid; e < K25_EH * K25_EW; e += KT_THREADS) {
            const int ly = e / K25_EW, lx = e - ly * K25_EW, gy = ty0 - 1 + ly, gx = tx0 - 1 + lx;
            const bool inner = ly >= 1 && ly <= KT_TH && lx >= 1 && lx <= KT_TW;
            int eff = 0;
            if ((GEO || inner) && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int64_t i = (int64_t)gy * W + gx;
                const int s = seg[i];
                if (s < 0 || s > nseg) nbad += inner;   // every pixel is the inner pixel of exactly one tile
                else if (s > 0 && (!mask || mask[i])) eff = s;
            }
            s_eff[ly][lx] = eff;
        }
        __syncthreads();

        const int y = ty0 + ry, xb = tx0 + cx;
        int l[KT_PXT], row[KT_PXT];   // the label and its LDS row (-1: none, commit to the global table)
        bool any = false;
#pragma unroll
        for (int j = 0; j < KT_PXT; j++) {
            l[j] = s_eff[ry + 1][cx + 1 + j];
            row[j] = -1;
            any = any || l[j] != 0;
        }
#pragma unroll
        for (int j = 0; j < KT_PXT; j++) {
            if (l[j] == 0) continue;
            if (j > 0 && l[j] == l[j - 1]) {
                row[j] = row[j - 1];
                continue;
            }
            int h = (int)(((unsigned)l[j] * 0x9E3779B1u) >> 26) & (K25_SLOTS - 1);
            for (int probe = 0; probe < K25_SLOTS; probe++) {   // the claim of K27 step 2, on a 32-bit key
                int k = s_key[h];
                if (k == 0) {
                    k = atomicCAS(&s_key[h], 0, l[j]);
                    if (k == 0) {
                        s_list[atomicAdd(&s_nocc, 1)] = h;   // at most K25_SLOTS rows are ever claimed
                        k = l[j];
                    }
                }
                if (k == l[j]) {
                    row[j] = h;
                    break;
                }
                h = (h + 1) & (K25_SLOTS - 1);
            }
        }

        // A thread walks its four pixels once per column group and commits at the last pixel of every maximal run of one label
        // (static indices only, so that the arrays stay in registers).  The LDS and the global commit are separate branches:
        // the first compiles to ds_* atomics, the second to global_* atomics.
        if (any) {
            {
                long long n = 0, sx = 0, sxx = 0, per = 0, x0 = 0;
#pragma unroll
                for (int j = 0; j < KT_PXT; j++) {
                    if (l[j] == 0) continue;
                    const long long x = xb + j;
                    if (n == 0) x0 = x;
                    n++;
                    if (GEO) {
                        sx += x;
                        sxx += x * x;
                        per += (s_eff[ry][cx + 1 + j] != l[j]) + (s_eff[ry + 2][cx + 1 + j] != l[j]) + (s_eff[ry + 1][cx + j] != l[j]) +
                               (s_eff[ry + 1][cx + 2 + j] != l[j]);
                    }
                    if (j + 1 < KT_PXT && l[j + 1] == l[j]) continue;
                    const long long yy = y;
                    const long long g[K25_GEO] = {n, n * yy, sx, n * yy * yy, sxx, sx * yy, yy, yy, x0, x, per};
                    if (row[j] >= 0) {
                        long long *d = s_tab + row[j] * C;
#pragma unroll
                        for (int c = 0; c < (GEO ? K25_GEO : 1); c++) k25_put(d + c, k25_kind(c), g[c]);
                    } else {
                        long long *d = table + (int64_t)l[j] * C;
#pragma unroll
                        for (int c = 0; c < (GEO ? K25_GEO : 1); c++) k25_put(d + c, k25_kind(c), g[c]);
                    }
                    n = sx = sxx = per = 0;
                }
            }

            const int64_t i0 = (int64_t)y * W + xb;   // the thread's first pixel; its pixels with l[j] != 0 are inside the image
            for (int p = 0; p < P; p++) {
                long long q[KT_PXT], q2[KT_PXT];
                if constexpr (sizeof(T) == 1) {
                    const uint8_t *src = reinterpret_cast<const uint8_t *>(pl.p[p]);
                    unsigned v[KT_PXT] = {0, 0, 0, 0};
                    if (vec) {   // W % 4 == 0 and the plane is 4-byte aligned: the four pixels are one aligned word inside the row
                        const unsigned w4 = *reinterpret_cast<const unsigned *>(src + i0);
#pragma unroll
                        for (int j = 0; j < KT_PXT; j++) v[j] = (w4 >> (8 * j)) & 0xffu;
                    } else {
#pragma unroll
                        for (int j = 0; j < KT_PXT; j++)
                            if (l[j] != 0) v[j] = src[i0 + j];
                    }
#pragma unroll
                    for (int j = 0; j < KT_PXT; j++) {
                        q[j] = v[j];
                        q2[j] = v[j] * v[j];
                    }
                } else {
                    const float *src = reinterpret_cast<const float *>(pl.p[p]);
                    float v[KT_PXT] = {0.f, 0.f, 0.f, 0.f};
                    if (vec) {   // W % 4 == 0 and the plane is 16-byte aligned
                        const float4 f4 = *reinterpret_cast<const float4 *>(src + i0);
                        v[0] = f4.x;
                        v[1] = f4.y;
                        v[2] = f4.z;
                        v[3] = f4.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < KT_PXT; j++)
                            if (l[j] != 0) v[j] = src[i0 + j];
                    }
#pragma unroll
                    for (int j = 0; j < KT_PXT; j++) {
                        q[j] = to_fixed40((double)v[j]);
                        q2[j] = k25_sq_fixed24((double)v[j]);
                    }
                }
                long long s1 = 0, s2 = 0, mn = INT64_MAX, mx = INT64_MIN;
#pragma unroll
                for (int j = 0; j < KT_PXT; j++) {
                    if (l[j] == 0) continue;
                    s1 += q[j];
                    s2 += q2[j];
                    mn = q[j] < mn ? q[j] : mn;
                    mx = q[j] > mx ? q[j] : mx;
                    if (j + 1 < KT_PXT && l[j + 1] == l[j]) continue;
                    const int c0 = K25_GEO + 4 * p;
                    if (row[j] >= 0) {
                        long long *d = s_tab + row[j] * C + c0;
                        k25_put(d, 0, s1);
                        k25_put(d + 1, 0, s2);
                        k25_put(d + 2, 1, mn);
                        k25_put(d + 3, 2, mx);
                    } else {
                        long long *d = table + (int64_t)l[j] * C + c0;
                        k25_put(d, 0, s1);
                        k25_put(d + 1, 0, s2);
                        k25_put(d + 2, 1, mn);
                        k25_put(d + 3, 2, mx);
                    }
                    s1 = s2 = 0;
                    mn = INT64_MAX;
                    mx = INT64_MIN;
                }
            }
        }
        __syncthreads();

        // flush: every occupied row once, consecutive lanes on consecutive columns; a row is left empty behind
        const int nocc = s_nocc;
        for (int e = tid; e < nocc * C; e += KT_THREADS) {
            const int r = s_list[e / C], c = e % C;
            const long long empty = k25_empty(c, H, W);
            const long long v = s_tab[r * C + c];
            if (v != empty) {
                s_tab[r * C + c] = empty;
                k25_put(table + (int64_t)s_key[r] * C + c, k25_kind(c), v);
            }
        }
        __syncthreads();
        if (tid < nocc) s_key[s_list[tid]] = 0;
        if (tid == 0) s_nocc = 0;
    }

    wg_count_commit<KT_THREADS>(bad, nbad);   // the labels outside 0 ... n_segments
}

extern "C" int rsseg_segment_features(rsseg_ctx *ctx, const int32_t *d_seg, int H, int W, int64_t n_segments, const void *const *d_planes, int P, int dtype,
                                      const uint8_t *d_mask, int flags, int64_t *d_table)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    RSCHK(kt_check_raster(ctx, "segment_features", d_seg, H, W, n_segments));
    const int64_t n = (int64_t)H * W;
    RSCHK(kt_check_planes(ctx, "segment_features", d_planes, P, 0));
    RSCHK(kt_check_dtype(ctx, "segment_features", dtype, "RSSEG_U8 or RSSEG_F32"));
    if (flags & ~RSSEG_OBJ_GEOMETRY) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_features: flags = %d holds unknown bits", flags);
    for (int p = 0; p < P; p++) RSCHK(kt_check_plane(ctx, "segment_features", d_planes, p, dtype));
    if (!d_table || ((uintptr_t)d_table & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_features: d_table null or not 8-byte aligned");
    {   // the largest coordinate moment is below H W max(H, W)^2
        const unsigned __int128 m = (unsigned __int128)std::max(H, W);
        if ((unsigned __int128)n * m * m >= ((unsigned __int128)1 << 63))
            return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "segment_features: H = %d, W = %d: H W max(H, W)^2 reaches 2^63, the coordinate moments leave int64", H, W);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RSCHK(ws_reserve(ctx, 256));
    RSCHK(pin_reserve(ctx, 256));
    unsigned long long *d_bad = (unsigned long long *)ctx->d_ws;
    kt_planes_t pl;
    memset(&pl, 0, sizeof(pl));
    for (int p = 0; p < P; p++) pl.p[p] = d_planes[p];
    const int vec = kt_vec(W, d_planes, P, dtype == RSSEG_U8 ? 3 : 15);
    const int C = K25_GEO + 4 * P;
    const int64_t rows = n_segments + 1;
    const int tiles_x = (W + KT_TW - 1) / KT_TW, tiles_y = (H + KT_TH - 1) / KT_TH;
    const int64_t ntiles = (int64_t)tiles_x * tiles_y;
    const size_t lds = sizeof(long long) * (size_t)K25_SLOTS * C;
    const bool geo = (flags & RSSEG_OBJ_GEOMETRY) != 0;
    HIPCHK(ctx, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), ctx->stream));
    {
        prof_scope ps(ctx, "segment_features");
        const unsigned gi = (unsigned)std::min<int64_t>(K25_MAX_BLOCKS, std::max<int64_t>(1, ceil_div64(rows * C, KT_THREADS)));
        hipLaunchKernelGGL(k25_init, dim3(gi), dim3(KT_THREADS), 0, ctx->stream, (long long *)d_table, rows, C, H, W);
        const dim3 grid((unsigned)std::min<int64_t>(K25_MAX_BLOCKS, ntiles)), block(KT_THREADS);
        const auto kernel = dtype == RSSEG_U8 ? (geo ? k25_features<uint8_t, true> : k25_features<uint8_t, false>)
                                              : (geo ? k25_features<float, true> : k25_features<float, false>);
        RSCHK(kt_launch(ctx, kernel, grid, block, lds, d_seg, d_mask, H, W, n_segments, pl, P, vec, tiles_x, ntiles, (long long *)d_table, d_bad));
        HIPCHK(ctx, hipGetLastError());
    }
    unsigned long long nbad = 0;
    RSCHK(kt_read(ctx, d_bad, sizeof(nbad), &nbad));
    return kt_bad_labels(ctx, "segment_features", nbad, n_segments);
}
