// K27 — the region adjacency graph of a segment map: one row per pair of segments that touch (4-connectivity), with the length
// of their shared border and, per uint8 plane, the summed absolute step across it (include/rsseg.h, rsseg_segment_adjacency).
// Everything is an integer sum, so the table has one right answer whatever the order the atomics land in; it is restated in
// NumPy in tests/adjacency_ref.py, to which the kernel is equal bit for bit (as a set of rows: their order is unspecified).
//
// A workgroup walks the 64 x 16 tiles of keyed_table.h (grid stride); a thread owns four consecutive pixels of a row.
//   1. The EFFECTIVE labels (K25's rule) of the tile and of one more column on its right and one more row below it are
//      staged in LDS (outside the image: 0).
//   2. A CROSSING is a pixel and its right or lower neighbour with effective labels a != b, both > 0; it belongs to the left /
//      upper pixel, so a crossing on a tile seam is counted by exactly one tile.  The pairs met in the tile share a table of
//      K27_SLOTS rows in LDS, found by open addressing on the 64-bit key min(a, b) << 32 | max(a, b) (K25's loop).  A thread adds
//      a RUN of equal crossings below its four pixels at once.  A pair that finds no LDS row commits straight to the global
//      table.
//   3. Every occupied row is flushed once per tile: one thread per row finds (or claims) the pair's row in the global
//      open-addressing table, adds the row's columns to it with 64-bit global atomics and puts the LDS row back to zero as it
//      reads it; the LDS table is therefore initialised once per workgroup.  (One thread per row, not one lane per column: the
//      flush waits for the lookup's round trip either way, and this form needs no barrier between the lookup and the adds.)
//   4. k27_compact writes the occupied rows of the global table to d_edges and counts them.
// The planes are read from global memory, and only by threads that own a crossing: under a superpixel map most threads own none.
// The tile's labels are all requested before the first is used, and the crossings to the right and below run one after the
// other so that their arrays share registers (80 VGPRs, six waves per SIMD): the pass waits on round trips, not on bandwidth.
//
// Capacity.  The global table has max_edges + max_edges / 2 + 64 rows.  More than max_edges distinct pairs are noticed either
// by a probe sequence that went round the whole table (the table is then full, so there are more pairs than rows) or by the
// compaction count; both end in RSSEG_ERR_UNSUPPORTED, and nothing else does.
#include <algorithm>

#include "keyed_table.h"

#define K27_SLOTS 128    // rows of the LDS table (a power of two); 128 x (1 key + 1 + 16) x 8 B = 18 KiB at P = 16
#define K27_MAX_BLOCKS 8192
#define K27_EW (KT_TW + 1)
#define K27_EH (KT_TH + 1)
#define K27_STAGE ((K27_EH * K27_EW + KT_THREADS - 1) / KT_THREADS)   // labels a thread stages per tile
static_assert(K27_SLOTS == 128, "the hash keeps the top seven bits of the product: change the shift with the row count");
static_assert(K27_SLOTS <= KT_THREADS && KT_TW * KT_TH == KT_THREADS * KT_PXT, "one thread per row of the list; four pixels per thread");

typedef unsigned long long k27_u64;

extern "C" void rsseg_segment_adjacency_plan(int P, int *tile_w, int *tile_h, int *lds_slots)
{
    (void)P;   // the plan does not depend on the plane count: the row gets wider, the table keeps its rows
    if (tile_w) *tile_w = KT_TW;
    if (tile_h) *tile_h = KT_TH;
    if (lds_slots) *lds_slots = K27_SLOTS;
}

// what the pass leaves for the host, at the head of the workspace
struct k27_head_t {
    k27_u64 bad;        // labels outside 0 ... n_segments
    k27_u64 count;      // occupied rows of the global table (k27_compact)
    unsigned full;      // a probe sequence went round the whole table
    unsigned pad;
};

__device__ __forceinline__ k27_u64 k27_mix(k27_u64 key)
{
    k27_u64 h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    return h * 0x9E3779B97F4A7C15ull;
}

// the row of `key` in the global table, claimed if the key is new; -1 when the table is full (or was found full by another
// thread).  Keys only ever go from 0 to their value, so a plain read that sees a key sees the final one.
__device__ __forceinline__ int64_t k27_global_row(k27_u64 *__restrict__ keys, int64_t cap, k27_u64 key, unsigned *full)
{
    int64_t s = (int64_t)__umul64hi(k27_mix(key), (k27_u64)cap);   // < cap
    for (int64_t probe = 0; probe < cap; probe++) {
        k27_u64 k = keys[s];
        if (k == 0) {
            k = atomicCAS(&keys[s], 0ull, key);
            if (k == 0) k = key;
        }
        if (k == key) return s;
        if ((probe & 255) == 255 && __hip_atomic_load(full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return -1;
        if (++s == cap) s = 0;
    }
    atomicExch(full, 1u);
    return -1;
}

// The four crossings of one direction of a thread's four pixels: with the pixel to the right (DOWN false) or with the pixel
// below (DOWN true).  key 0: no crossing.  The two directions run one after the other, so that their arrays share registers.
template <bool DOWN>
__device__ __forceinline__ void k27_group(const int (*s_eff)[K27_EW], k27_u64 *s_key, int *s_list, int *s_nocc, long long *s_tab, int C, int P, int vec, int W,
                                          int ry, int cx, int64_t i0, const kt_planes_t &pl, k27_u64 *__restrict__ gkeys, long long *__restrict__ gvals,
                                          int64_t cap, unsigned *full)
{
    k27_u64 key[KT_PXT];
    int row[KT_PXT];          // >= 0: the LDS row; -1: the global row grow[c]; -2: nothing to add
    int64_t grow[KT_PXT];
    bool any = false;
#pragma unroll
    for (int c = 0; c < KT_PXT; c++) {
        const int a = s_eff[ry][cx + c], b = DOWN ? s_eff[ry + 1][cx + c] : s_eff[ry][cx + c + 1];
        key[c] = 0;
        if (a > 0 && b > 0 && a != b) key[c] = ((k27_u64)(unsigned)min(a, b) << 32) | (unsigned)max(a, b);
        row[c] = -2;
        grow[c] = -1;
        any = any || key[c] != 0;
    }
    if (!any) return;
#pragma unroll
    for (int c = 0; c < KT_PXT; c++) {
        if (key[c] == 0) continue;
        if (DOWN && c > 0 && key[c] == key[c - 1]) {   // a run below the thread's pixels
            row[c] = row[c - 1];
            grow[c] = grow[c - 1];
            continue;
        }
        int h = (int)(k27_mix(key[c]) >> 57) & (K27_SLOTS - 1);
        for (int probe = 0; probe < K27_SLOTS; probe++) {   // the claim of K25 step 2, on a 64-bit key; a shared template cost the overflow case 0.25 %
            k27_u64 k = s_key[h];
            if (k == 0) {
                k = atomicCAS(&s_key[h], 0ull, key[c]);
                if (k == 0) {
                    s_list[atomicAdd(s_nocc, 1)] = h;   // at most K27_SLOTS rows are ever claimed
                    k = key[c];
                }
            }
            if (k == key[c]) {
                row[c] = h;
                break;
            }
            h = (h + 1) & (K27_SLOTS - 1);
        }
        if (row[c] == -2) {
            grow[c] = k27_global_row(gkeys, cap, key[c], full);
            if (grow[c] >= 0) row[c] = -1;
        }
    }

    // The crossings are walked once per column, and a run commits at its last crossing (static indices only, so that the arrays
    // stay in registers).  The LDS and the global commit are separate branches: ds_* and global_* atomics.
    {
        long long n = 0;
#pragma unroll
        for (int c = 0; c < KT_PXT; c++) {
            if (key[c] == 0) continue;
            n++;
            if (DOWN && c + 1 < KT_PXT && key[c + 1] == key[c]) continue;
            if (row[c] >= 0) atomicAdd(reinterpret_cast<k27_u64 *>(s_tab + row[c] * C), (k27_u64)n);
            else if (row[c] == -1) atomicAdd(reinterpret_cast<k27_u64 *>(gvals + grow[c] * C), (k27_u64)n);
            n = 0;
        }
    }
    for (int p = 0; p < P; p++) {   // a pixel of a crossing is inside the image, and so is its neighbour
        const uint8_t *src = reinterpret_cast<const uint8_t *>(pl.p[p]);
        int a[KT_PXT] = {0, 0, 0, 0}, b[KT_PXT] = {0, 0, 0, 0};
        if (vec) {   // W % 4 == 0 and the plane is 4-byte aligned: four pixels are one aligned word inside the row
            const unsigned w4 = *reinterpret_cast<const unsigned *>(src + i0);
            unsigned o4;
            if (DOWN) o4 = *reinterpret_cast<const unsigned *>(src + i0 + W);
            else o4 = (w4 >> 8) | (key[KT_PXT - 1] != 0 ? (unsigned)src[i0 + KT_PXT] << 24 : 0u);
#pragma unroll
            for (int j = 0; j < KT_PXT; j++) {
                a[j] = (int)((w4 >> (8 * j)) & 0xffu);
                b[j] = (int)((o4 >> (8 * j)) & 0xffu);
            }
        } else {
#pragma unroll
            for (int j = 0; j < KT_PXT; j++)
                if (key[j] != 0) {
                    a[j] = src[i0 + j];
                    b[j] = DOWN ? src[i0 + W + j] : src[i0 + j + 1];
                }
        }
        long long s = 0;
#pragma unroll
        for (int c = 0; c < KT_PXT; c++) {
            if (key[c] == 0) continue;
            const int d = a[c] - b[c];
            s += d < 0 ? -d : d;
            if (DOWN && c + 1 < KT_PXT && key[c + 1] == key[c]) continue;
            if (s != 0) {
                if (row[c] >= 0) atomicAdd(reinterpret_cast<k27_u64 *>(s_tab + row[c] * C + 1 + p), (k27_u64)s);
                else if (row[c] == -1) atomicAdd(reinterpret_cast<k27_u64 *>(gvals + grow[c] * C + 1 + p), (k27_u64)s);
            }
            s = 0;
        }
    }
}

__global__ __launch_bounds__(KT_THREADS) void k27_adjacency(const int *__restrict__ seg, const uint8_t *__restrict__ mask, int H, int W, int64_t nseg,
                                                             kt_planes_t pl, int P, int vec, int tiles_x, int64_t ntiles, k27_u64 *__restrict__ gkeys,
                                                             long long *__restrict__ gvals, int64_t cap, k27_head_t *__restrict__ head)
{
    extern __shared__ __align__(16) unsigned char k27_lds[];
    __shared__ int s_eff[K27_EH][K27_EW];      // effective labels of the tile, one more column and one more row
    __shared__ k27_u64 s_key[K27_SLOTS];       // 0: free, else the pair the row belongs to
    __shared__ int s_list[K27_SLOTS];          // the occupied rows, in the order they were claimed
    __shared__ int s_nocc;
    long long *s_tab = reinterpret_cast<long long *>(k27_lds);   // [K27_SLOTS][C]: length, then the contrast of every plane
    const int C = 1 + P, tid = threadIdx.x;
    for (int e = tid; e < K27_SLOTS * C; e += KT_THREADS) s_tab[e] = 0;
    if (tid < K27_SLOTS) s_key[tid] = 0;
    const int ry = kt_ry(tid), cx = kt_cx(tid);
    unsigned nbad = 0;

    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx0 = (int)(t % tiles_x) * KT_TW, ty0 = (int)(t / tiles_x) * KT_TH;
        __syncthreads();   // the table is empty, the list of the previous tile and its labels are no longer read
        if (tid == 0) s_nocc = 0;
        {   // every load of the tile's labels is issued before the first is used
            int sv[K27_STAGE];
            uint8_t mv[K27_STAGE];
#pragma unroll
            for (int it = 0; it < K27_STAGE; it++) {
                const int e = tid + it * KT_THREADS, ly = e / K27_EW, lx = e - ly * K27_EW, gy = ty0 + ly, gx = tx0 + lx;
                const bool in = e < K27_EH * K27_EW && gy < H && gx < W;
                const int64_t i = (int64_t)gy * W + gx;
                sv[it] = in ? seg[i] : 0;
                mv[it] = in && mask ? mask[i] : (uint8_t)1;
            }
#pragma unroll
            for (int it = 0; it < K27_STAGE; it++) {
                const int e = tid + it * KT_THREADS, ly = e / K27_EW, lx = e - ly * K27_EW;
                if (e >= K27_EH * K27_EW) continue;
                int eff = 0;   // K25's rule, written out with the claim
                if (sv[it] < 0 || sv[it] > nseg) nbad += ly < KT_TH && lx < KT_TW;   // every pixel is the inner pixel of exactly one tile
                else if (mv[it]) eff = sv[it];
                s_eff[ly][lx] = eff;
            }
        }
        __syncthreads();

        const int64_t i0 = (int64_t)(ty0 + ry) * W + tx0 + cx;   // the thread's first pixel
        k27_group<false>(s_eff, s_key, s_list, &s_nocc, s_tab, C, P, vec, W, ry, cx, i0, pl, gkeys, gvals, cap, &head->full);
        k27_group<true>(s_eff, s_key, s_list, &s_nocc, s_tab, C, P, vec, W, ry, cx, i0, pl, gkeys, gvals, cap, &head->full);
        __syncthreads();

        // flush: one thread per occupied row finds the pair's global row and adds the row's columns to it; the LDS row is left
        // zero and free behind
        if (tid < s_nocc) {
            const int r = s_list[tid];
            const int64_t g = k27_global_row(gkeys, cap, s_key[r], &head->full);
            for (int c = 0; c < C; c++) {
                const long long v = s_tab[r * C + c];
                if (v != 0) {
                    s_tab[r * C + c] = 0;
                    if (g >= 0) atomicAdd(reinterpret_cast<k27_u64 *>(gvals + g * C + c), (k27_u64)v);
                }
            }
            s_key[r] = 0;
        }
    }

    wg_count_commit<KT_THREADS>(&head->bad, nbad);   // the labels outside 0 ... n_segments
}

// The occupied rows of the global table to d_edges as (a, b, length, contrasts): a workgroup takes 256 rows at a time, counts
// its occupied ones and draws their places with ONE atomic; places past max_edges are counted and not written.
__global__ __launch_bounds__(KT_THREADS) void k27_compact(const k27_u64 *__restrict__ gkeys, const long long *__restrict__ gvals, int64_t cap, int C,
                                                           int64_t max_edges, long long *__restrict__ edges, k27_head_t *__restrict__ head)
{
    __shared__ unsigned s_cnt[KT_THREADS / WAVE];
    __shared__ k27_u64 s_base;
    const int tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
    const int64_t chunks = (cap + KT_THREADS - 1) / KT_THREADS;
    for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const int64_t s = ch * KT_THREADS + tid;
        const k27_u64 key = s < cap ? gkeys[s] : 0ull;
        const k27_u64 bal = __ballot(key != 0);
        const unsigned before = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        if (tid == 0) {
            unsigned tot = 0;
            for (int w = 0; w < KT_THREADS / WAVE; w++) tot += s_cnt[w];
            s_base = tot ? atomicAdd(&head->count, (k27_u64)tot) : 0ull;
        }
        __syncthreads();
        if (key != 0) {
            unsigned off = before;
            for (int w = 0; w < wave; w++) off += s_cnt[w];
            const int64_t at = (int64_t)s_base + off;
            if (at < max_edges) {
                long long *o = edges + at * (2 + C);
                o[0] = (long long)(key >> 32);
                o[1] = (long long)(key & 0xffffffffull);
                for (int c = 0; c < C; c++) o[2 + c] = gvals[s * C + c];
            }
        }
        __syncthreads();   // s_cnt and s_base are rewritten by the next chunk
    }
}

extern "C" int rsseg_segment_adjacency(rsseg_ctx *ctx, const int32_t *d_seg, int H, int W, int64_t n_segments, const uint8_t *d_mask,
                                       const uint8_t *const *d_planes, int P, int64_t max_edges, int64_t *d_edges, int64_t *n_edges)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (n_edges) *n_edges = 0;
    RSCHK(kt_check_raster(ctx, "segment_adjacency", d_seg, H, W, n_segments));
    RSCHK(kt_check_planes(ctx, "segment_adjacency", d_planes, P, 0));
    for (int p = 0; p < P; p++) RSCHK(kt_check_plane_u8(ctx, "segment_adjacency", d_planes, p));
    if (max_edges < 0 || max_edges > ((int64_t)1 << 33))   // at most 2 H W - H - W < 2^32 crossings exist
        return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_adjacency: max_edges = %lld is not in 0 ... 2^33", (long long)max_edges);
    if (max_edges > 0 && (!d_edges || ((uintptr_t)d_edges & 7)))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_adjacency: d_edges null or not 8-byte aligned");
    if (!n_edges) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_adjacency: n_edges is null");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int C = 1 + P;
    const int64_t cap = max_edges + max_edges / 2 + 64;
    const size_t head_bytes = 256, key_bytes = sizeof(k27_u64) * (size_t)cap, val_bytes = sizeof(long long) * (size_t)cap * C;
    RSCHK(ws_reserve(ctx, head_bytes + key_bytes + val_bytes));
    RSCHK(pin_reserve(ctx, 256));
    k27_head_t *d_head = (k27_head_t *)ctx->d_ws;
    k27_u64 *d_keys = (k27_u64 *)(ctx->d_ws + head_bytes);
    long long *d_vals = (long long *)(ctx->d_ws + head_bytes + key_bytes);
    kt_planes_t pl;
    memset(&pl, 0, sizeof(pl));
    for (int p = 0; p < P; p++) pl.p[p] = d_planes[p];
    const int vec = kt_vec(W, reinterpret_cast<const void *const *>(d_planes), P, 3);
    const int tiles_x = (W + KT_TW - 1) / KT_TW, tiles_y = (H + KT_TH - 1) / KT_TH;
    const int64_t ntiles = (int64_t)tiles_x * tiles_y;
    const size_t lds = sizeof(long long) * (size_t)K27_SLOTS * C;
    {
        prof_scope ps(ctx, "segment_adjacency");
        HIPCHK(ctx, hipMemsetAsync(ctx->d_ws, 0, head_bytes + key_bytes + val_bytes, ctx->stream));
        const dim3 grid((unsigned)std::min<int64_t>(K27_MAX_BLOCKS, ntiles)), block(KT_THREADS);
        RSCHK(kt_launch(ctx, k27_adjacency, grid, block, lds, d_seg, d_mask, H, W, n_segments, pl, P, vec, tiles_x, ntiles, d_keys, d_vals, cap, d_head));
        HIPCHK(ctx, hipGetLastError());
    }
    {
        prof_scope ps(ctx, "segment_adjacency_compact");
        const dim3 grid((unsigned)std::min<int64_t>(K27_MAX_BLOCKS, ceil_div64(cap, KT_THREADS))), block(KT_THREADS);
        RSCHK(kt_launch(ctx, k27_compact, grid, block, 0, d_keys, d_vals, cap, C, max_edges, (long long *)d_edges, d_head));
        HIPCHK(ctx, hipGetLastError());
    }
    k27_head_t head;
    RSCHK(kt_read(ctx, d_head, sizeof(head), &head));
    RSCHK(kt_bad_labels(ctx, "segment_adjacency", head.bad, n_segments));
    if (head.full || head.count > (k27_u64)max_edges)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "segment_adjacency: the raster holds more than max_edges = %lld distinct pairs of adjacent segments",
                       (long long)max_edges);
    *n_edges = (int64_t)head.count;
    return RSSEG_OK;
}
