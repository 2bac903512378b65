// K20 — clean-up of a per-pixel class map (uint8, H x W): k x k majority (mode) filter and multi-class sieve.  Neither has a
// counterpart in the reference, whose advanced_post_processing cleans binary masks only (K12); the semantics are this
// project's own and are restated in tests/postclass_ref.py.
//
// Majority filter.  The window is k x k (k odd, 3 ... 15), centred on the pixel and CLIPPED to the image: cells outside do not
// vote.  `ignore` pixels never vote and are never changed; `fill` pixels never vote and take their window's winner when the
// window has a voter; with fill_only every other pixel keeps its value.  The winner is the label with the most votes; on a tie
// the centre keeps its label when that label votes and is among the maxima, otherwise the smallest tied label wins.
//   Counting: a window holds at most 15 x 15 = 225 votes, so a byte per label never carries and eight labels ("a group") share
// one 64-bit word: the vote of value v for the group starting at `base` is 1 << 8 (v - base), the horizontal sum of k votes
// and the vertical sum of k row terms are plain 64-bit adds, and so are their sliding forms (add the entering term, subtract
// the leaving one: a byte only ever loses what it holds).  The kernel is the K5-K8 tile walk (window_tile.h: 256 x 32 tile in
// LDS, 4 columns x 8 rows per thread, a K-deep register ring of row terms) with that 64-bit term, repeated over the staged
// tile for every group of eight labels that occurs (a 32-bit mask from a 256-bin histogram: labels 0..7 cost one walk,
// {0, 200, 255} three).  Across the groups a pixel carries one 32-bit key, count << 9 | centre << 8 | 255 - label, whose
// maximum IS the winner under the tie rule.  The tile is staged with edge replication only to keep the loads in bounds:
// rows outside the plane contribute no row term and columns outside the image no vote.
//   Rows form: the plane holds Hin rows, image rows [img_y0, img_y0 + Hin); rows [y0, y1) of it are produced.  The window is
// clipped against the IMAGE's first and last row, so a row the window reaches inside the image must be in the plane.
//   HBM traffic: the plane once in (halo re-reads are L2 hits), once out, and one more read for the histogram when the
// caller gives no group mask.
//
// Sieve.  Pixels are connected when they are 8-neighbours (or 4-), hold the SAME label, and that label is not `ignore`;
// every component of fewer than min_area pixels becomes removed_value.  The union-find of K12 (cc.h) with the predicate
// q[i] == q[j] labels all classes in one pass: init, union with the W / NW / N / NE neighbours, flatten + count, filter.
// The result depends on connectivity and areas only, so it is deterministic whatever order the atomics land in.
#include "cc.h"
#include "common.h"

// ---- tile geometry of the majority filter (the numbers of K5-K8; window_tile.h is written against these names) ----
#define TW 256                      // output columns per workgroup
#define TH 32                       // output rows per workgroup
#define CPT 4                       // columns per thread
#define RPT 8                       // output rows per thread
#define TPAD 4                      // default staged columns left / right of the tile; windows above 9 stage 8 (k20_majority)
#define TSTRIDE (TW + 2 * TPAD)
#define WIN_MAXP 8
#include "window_tile.h"

#define K20_THREADS 256

static inline unsigned k20_grid(int64_t n) { return (unsigned)std::min<int64_t>(65535 * 16, std::max<int64_t>(1, ceil_div64(n, K20_THREADS))); }

// adds every thread's a and b into cnt[0] and cnt[1]: one atomic per counter and WORKGROUP (every thread must call it)
__device__ __forceinline__ void k20_commit2(unsigned long long *cnt, unsigned a, unsigned b)
{
    __shared__ unsigned s_a[K20_THREADS / WAVE], s_b[K20_THREADS / WAVE];
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane_id() == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < K20_THREADS / WAVE; w++) { a += s_a[w]; b += s_b[w]; }
        if (a) atomicAdd(&cnt[0], (unsigned long long)a);
        if (b) atomicAdd(&cnt[1], (unsigned long long)b);
    }
}

// 256-bin histogram of a uint8 plane.  A thread counts runs of equal values and commits a run when it ends, so a smooth class
// map costs far fewer LDS atomics than pixels; one histogram per wave keeps the waves off each other's bins.
__global__ __launch_bounds__(K20_THREADS) void k20_hist(const uint8_t *__restrict__ q, int64_t n, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned h[K20_THREADS / WAVE][256];
    for (int w = 0; w < K20_THREADS / WAVE; w++) h[w][threadIdx.x] = 0;
    __syncthreads();
    unsigned *mine = h[threadIdx.x >> 6];
    const int64_t lead = (int64_t)((16 - ((uintptr_t)q & 15)) & 15), head = lead < n ? lead : n, nv = (n - head) / 16;
    const rs_u4v *qv = reinterpret_cast<const rs_u4v *>(q + head);
    int cur = -1;
    unsigned run = 0;
    for (int64_t i = (int64_t)blockIdx.x * K20_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * K20_THREADS) {
        const rs_u4v v = qv[i];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int b = (int)((v[e >> 2] >> (8 * (e & 3))) & 255u);
            if (b != cur) {
                if (run) atomicAdd(&mine[cur], run);
                cur = b;
                run = 0;
            }
            run++;
        }
    }
    if (run) atomicAdd(&mine[cur], run);
    // the unaligned head and the tail of fewer than 16 bytes
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + 16 * nv;
        for (int64_t i = threadIdx.x; i < head + (n - tail0); i += K20_THREADS) atomicAdd(&mine[q[i < head ? i : tail0 + (i - head)]], 1u);
    }
    __syncthreads();
    unsigned s = 0;
    for (int w = 0; w < K20_THREADS / WAVE; w++) s += h[w][threadIdx.x];
    if (s) atomicAdd(&hist[threadIdx.x], (unsigned long long)s);
}

// ---- majority filter ----
template <int K>
__global__ __launch_bounds__(256) void k20_majority(const uint8_t *__restrict__ q, int Hin, int W, int y0, int nrows, int ignore, int fill, int fill_only,
                                                    uint32_t groups, uint8_t *__restrict__ out, unsigned long long *__restrict__ cnt, tile_map tm)
{
    constexpr int R = K / 2;
    constexpr int PADW = (R + 3) / 4, PAD = 4 * PADW;   // staged columns either side of the tile: 4 up to k = 9, 8 beyond
    constexpr int STRIDE = TW + 2 * PAD;
    constexpr int NW = 1 + 2 * PADW, NV = 4 * NW;       // dwords / values a thread reads of a tile row: columns cx - PAD ... cx + 3 + PAD
    __shared__ __align__(16) uint8_t tile[(TH + 2 * R) * STRIDE];
    tile_pos t;
    if (!stage_tile<uint8_t, R, PAD>(tile, q, Hin, W, y0, BORDER_REPLICATE, tm, t)) return;   // whole workgroup: uniform
    unsigned changed = 0, unfilled = 0;
    if (t.x0 + t.cx < W && t.ty0 + t.ry < nrows) {
        // the 4 centre pixels of output row i of this thread, one byte each
        auto centre = [&](int i) { return *reinterpret_cast<const uint32_t *>(tile + (t.ry + i + R) * STRIDE + t.cx + PAD); };
        // bit e: column x0 + cx - PAD + e is inside the image
        uint32_t colok = 0;
#pragma unroll
        for (int e = 0; e < NV; e++) {
            const int c = t.x0 + t.cx - PAD + e;
            colok |= (uint32_t)(c >= 0 && c < W) << e;
        }
        uint32_t key[RPT][CPT];   // count << 9 | (label is the centre's) << 8 | 255 - label: the maximum is the winner
#pragma unroll
        for (int i = 0; i < RPT; i++)
#pragma unroll
            for (int c = 0; c < CPT; c++) key[i][c] = 0;
        for (uint32_t gm = groups; gm; gm &= gm - 1) {
            const int base = 8 * __builtin_ctz(gm);
            uint64_t ring[K][CPT], S[CPT];
#pragma unroll
            for (int c = 0; c < CPT; c++) S[c] = 0;
#pragma unroll
            for (int j = 0; j < RPT + 2 * R; j++) {
                const int prow = y0 + t.ty0 + t.ry + j - R;   // the plane row in tile row ry + j (the same for a whole wave)
                uint64_t h[CPT];
                if (prow >= 0 && prow < Hin) {
                    const uint32_t *wp = reinterpret_cast<const uint32_t *>(tile + (t.ry + j) * STRIDE + t.cx);
                    uint64_t vote[NV];
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const uint32_t d = wp[w];
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const int e = 4 * w + b, v = (int)((d >> (8 * b)) & 255u);
                            const bool votes = v != ignore && v != fill && ((colok >> e) & 1u) && (unsigned)(v - base) < 8u;
                            vote[e] = votes ? 1ull << (8 * ((v - base) & 7)) : 0ull;
                        }
                    }
                    h[0] = vote[PAD - R];
#pragma unroll
                    for (int d = 1; d < K; d++) h[0] += vote[PAD - R + d];
#pragma unroll
                    for (int c = 1; c < CPT; c++) h[c] = h[c - 1] + vote[PAD - R + c - 1 + K] - vote[PAD - R + c - 1];
                } else {
#pragma unroll
                    for (int c = 0; c < CPT; c++) h[c] = 0;
                }
#pragma unroll
                for (int c = 0; c < CPT; c++) {
                    S[c] += h[c];
                    if (j >= K) S[c] -= ring[j % K][c];   // the row term that left the window
                    ring[j % K][c] = h[c];
                }
                if (j >= 2 * R) {
                    const int i = j - 2 * R;
                    const uint32_t cw = centre(i);
#pragma unroll
                    for (int c = 0; c < CPT; c++) {
                        const uint32_t lo = (uint32_t)S[c], hi = (uint32_t)(S[c] >> 32);
                        uint32_t best = key[i][c];
#pragma unroll
                        for (int b = 0; b < 8; b++) {
                            const uint32_t n = ((b < 4 ? lo : hi) >> (8 * (b & 3))) & 255u;
                            const uint32_t kb = (n << 9) | (uint32_t)(255 - base - b);
                            best = kb > best ? kb : best;
                        }
                        const int cv = (int)((cw >> (8 * c)) & 255u);
                        if ((unsigned)(cv - base) < 8u && cv != ignore && cv != fill) {
                            const uint32_t n = (uint32_t)(S[c] >> (8 * (cv - base))) & 255u;   // >= 1: the centre votes for itself
                            const uint32_t kc = (n << 9) | 256u | (uint32_t)(255 - cv);
                            best = kc > best ? kc : best;
                        }
                        key[i][c] = best;
                    }
                }
            }
        }
        const row_store<uint8_t> store(out, W);
#pragma unroll
        for (int i = 0; i < RPT; i++) {
            const int orow = t.ty0 + t.ry + i;
            if (orow < nrows) {
                const uint32_t cw = centre(i);
                int o[CPT];
#pragma unroll
                for (int c = 0; c < CPT; c++) {
                    const int cv = (int)((cw >> (8 * c)) & 255u);
                    const int votes = (int)(key[i][c] >> 9), win = 255 - (int)(key[i][c] & 255u);
                    int r = cv;
                    if (cv == fill) r = votes ? win : cv;
                    else if (cv != ignore && !fill_only) r = win;
                    o[c] = r;
                    if (t.x0 + t.cx + c < W) {
                        changed += r != cv;
                        unfilled += cv == fill && r == fill;
                    }
                }
                store(orow, t.x0 + t.cx, o);
            }
        }
    }
    k20_commit2(cnt, changed, unfilled);
}

// ---- multi-class sieve ----
__global__ __launch_bounds__(K20_THREADS) void k20_cc_init(const uint8_t *__restrict__ q, int64_t n, int ignore, int *__restrict__ L, int *__restrict__ area)
{
    for (int64_t i = (int64_t)blockIdx.x * K20_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * K20_THREADS) {
        L[i] = (int)q[i] != ignore ? (int)i : -1;
        area[i] = 0;
    }
}
__global__ __launch_bounds__(K20_THREADS) void k20_cc_union(const uint8_t *__restrict__ q, int H, int W, int ignore, int diagonals, int *__restrict__ L)
{
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * K20_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * K20_THREADS) {
        const int v = q[i];
        if (v == ignore) continue;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        if (x > 0 && q[i - 1] == v) cc_union(L, (int)i, (int)i - 1);
        if (y > 0) {
            if (q[i - W] == v) cc_union(L, (int)i, (int)(i - W));
            if (diagonals && x > 0 && q[i - W - 1] == v) cc_union(L, (int)i, (int)(i - W - 1));
            if (diagonals && x + 1 < W && q[i - W + 1] == v) cc_union(L, (int)i, (int)(i - W + 1));
        }
    }
}
__global__ __launch_bounds__(K20_THREADS) void k20_cc_count(int64_t n, int *__restrict__ L, int *__restrict__ area)
{
    for (int64_t i = (int64_t)blockIdx.x * K20_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * K20_THREADS) {
        if (L[i] < 0) continue;
        const int r = cc_find(L, (int)i);
        L[i] = r;                      // roots never change after the union pass, so flattening here is safe
        atomicAdd(&area[r], 1);
    }
}
__global__ __launch_bounds__(K20_THREADS) void k20_cc_filter(const uint8_t *__restrict__ q, int64_t n, const int *__restrict__ L, const int *__restrict__ area,
                                                             int min_area, int removed_value, uint8_t *__restrict__ out, unsigned long long *__restrict__ cnt)
{
    unsigned removed = 0;
    for (int64_t i = (int64_t)blockIdx.x * K20_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * K20_THREADS) {
        const int r = L[i];
        // a pixel flattened before its root received its last child still points INTO its component: walk up (read-only)
        const bool small = r >= 0 && area[cc_find(L, r)] < min_area;
        out[i] = small ? (uint8_t)removed_value : q[i];
        removed += small;
    }
    k20_commit2(cnt, removed, 0u);
}

// q[i] = to where q[i] == from, in place (clean_class_map: the holes no pass could fill become nodata)
__global__ __launch_bounds__(K20_THREADS) void k20_replace(uint8_t *__restrict__ q, int64_t n, int from, int to, unsigned long long *__restrict__ cnt)
{
    unsigned hits = 0;
    for (int64_t i = (int64_t)blockIdx.x * K20_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * K20_THREADS)
        if ((int)q[i] == from) {
            q[i] = (uint8_t)to;
            hits++;
        }
    k20_commit2(cnt, hits, 0u);
}

extern "C" int rsseg_replace_u8(rsseg_ctx *ctx, uint8_t *d_q, int64_t n, int from, int to, int64_t *n_replaced)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_q) return rs_fail(ctx, RSSEG_ERR_INVALID, "replace_u8: d_q is null");
    if (n < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "replace_u8: n = %lld is negative", (long long)n);
    if (from < 0 || from > 255) return rs_fail(ctx, RSSEG_ERR_INVALID, "replace_u8: from = %d is not in 0 ... 255", from);
    if (to < 0 || to > 255) return rs_fail(ctx, RSSEG_ERR_INVALID, "replace_u8: to = %d is not in 0 ... 255", to);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RSCHK(ws_reserve(ctx, 64));
    RSCHK(pin_reserve(ctx, 64));
    unsigned long long *d_cnt = (unsigned long long *)ctx->d_ws;
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), ctx->stream));
    if (n) hipLaunchKernelGGL(k20_replace, dim3(k20_grid(n)), dim3(K20_THREADS), 0, ctx->stream, d_q, n, from, to, d_cnt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    if (n_replaced) *n_replaced = (int64_t)((const unsigned long long *)ctx->h_pin)[0];
    return RSSEG_OK;
}

static int k20_special(rsseg_ctx *ctx, const char *what, const char *name, int v)
{
    if (v < -1 || v > 255) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: %s = %d is neither -1 (none) nor a value in 0 ... 255", what, name, v);
    return RSSEG_OK;
}

extern "C" int rsseg_hist_u8(rsseg_ctx *ctx, const uint8_t *d_q, int64_t n, int64_t *counts)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_q) return rs_fail(ctx, RSSEG_ERR_INVALID, "hist_u8: d_q is null");
    if (!counts) return rs_fail(ctx, RSSEG_ERR_INVALID, "hist_u8: counts is null");
    if (n < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "hist_u8: n = %lld is negative", (long long)n);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RSCHK(ws_reserve(ctx, 256 * sizeof(unsigned long long)));
    RSCHK(pin_reserve(ctx, 256 * sizeof(unsigned long long)));
    unsigned long long *d_hist = (unsigned long long *)ctx->d_ws;
    HIPCHK(ctx, hipMemsetAsync(d_hist, 0, 256 * sizeof(unsigned long long), ctx->stream));
    if (n) {
        prof_scope ps(ctx, "class_hist");
        const unsigned g = (unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, ceil_div64(n, 16 * K20_THREADS)));
        hipLaunchKernelGGL(k20_hist, dim3(g), dim3(K20_THREADS), 0, ctx->stream, d_q, n, d_hist);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_hist, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    for (int b = 0; b < 256; b++) counts[b] = (int64_t)((const unsigned long long *)ctx->h_pin)[b];
    return RSSEG_OK;
}

extern "C" int rsseg_majority_u8(rsseg_ctx *ctx, const uint8_t *d_q, int Hin, int W, int y0, int y1, int img_y0, int img_H, int k, int ignore, int fill,
                                 int fill_only, uint32_t group_mask, uint8_t *d_out, int64_t *n_changed, int64_t *n_unfilled)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_q) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: d_q is null");
    if (!d_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: d_out is null");
    if (!n_changed) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: n_changed is null");
    if (!n_unfilled) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: n_unfilled is null");
    if (d_q == d_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: d_out is d_q (in-place not supported)");
    if (k < 3 || k > 15 || k % 2 == 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: k = %d is not an odd number in 3 ... 15", k);
    RSCHK(k20_special(ctx, "majority", "ignore", ignore));
    RSCHK(k20_special(ctx, "majority", "fill", fill));
    if (ignore >= 0 && ignore == fill) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: ignore and fill are both %d", fill);
    if (Hin < 1 || W < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: Hin = %d, W = %d: both must be at least 1", Hin, W);
    if (y0 < 0 || y1 > Hin || y0 > y1) return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: rows [%d,%d) are not rows of a %d-row plane", y0, y1, Hin);
    if (img_y0 < 0 || (int64_t)img_y0 + Hin > img_H)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: img_y0 = %d, img_H = %d: the %d-row plane is not inside the image", img_y0, img_H, Hin);
    const int R = k / 2;
    if (y0 < y1) {
        // every image row the windows of rows [y0, y1) reach must be in the plane
        const int64_t lo = std::max<int64_t>(0, (int64_t)img_y0 + y0 - R), hi = std::min<int64_t>(img_H, (int64_t)img_y0 + y1 + R);
        if (lo < img_y0 || hi > (int64_t)img_y0 + Hin)
            return rs_fail(ctx, RSSEG_ERR_INVALID, "majority: rows [%d,%d) of a %d-row stripe need %d halo rows on a side that is not an image edge", y0, y1,
                           Hin, R);
    }
    *n_changed = 0;
    *n_unfilled = 0;
    if (y0 == y1) return RSSEG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!group_mask) {
        int64_t counts[256];
        RSCHK(rsseg_hist_u8(ctx, d_q, (int64_t)Hin * W, counts));
        for (int b = 0; b < 256; b++)
            if (counts[b] && b != ignore && b != fill) group_mask |= 1u << (b >> 3);
    }
    RSCHK(ws_reserve(ctx, 64));
    RSCHK(pin_reserve(ctx, 64));
    unsigned long long *d_cnt = (unsigned long long *)ctx->d_ws;
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), ctx->stream));
    {
        prof_scope ps(ctx, "majority");
        const stencil_launch sl(y1 - y0, W);
#define K20_GO(KK)                                                                                                                              \
    case KK:                                                                                                                                    \
        hipLaunchKernelGGL((k20_majority<KK>), sl.grid, dim3(256), 0, ctx->stream, d_q, Hin, W, y0, y1 - y0, ignore, fill, fill_only ? 1 : 0, \
                           group_mask, d_out, d_cnt, sl.tm);                                                                                    \
        break;
        switch (k) {
            K20_GO(3) K20_GO(5) K20_GO(7) K20_GO(9) K20_GO(11) K20_GO(13) K20_GO(15)
        }
#undef K20_GO
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_cnt, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    *n_changed = (int64_t)((const unsigned long long *)ctx->h_pin)[0];
    *n_unfilled = (int64_t)((const unsigned long long *)ctx->h_pin)[1];
    return RSSEG_OK;
}

extern "C" int rsseg_sieve_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int min_area, int connectivity, int ignore, int removed_value,
                              uint8_t *d_out, int64_t *n_removed)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_q) return rs_fail(ctx, RSSEG_ERR_INVALID, "sieve: d_q is null");
    if (!d_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "sieve: d_out is null");
    if (!n_removed) return rs_fail(ctx, RSSEG_ERR_INVALID, "sieve: n_removed is null");
    if (d_q == d_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "sieve: d_out is d_q (in-place not supported)");
    if (connectivity != 4 && connectivity != 8) return rs_fail(ctx, RSSEG_ERR_INVALID, "sieve: connectivity = %d is neither 4 nor 8", connectivity);
    RSCHK(k20_special(ctx, "sieve", "ignore", ignore));
    if (removed_value < 0 || removed_value > 255) return rs_fail(ctx, RSSEG_ERR_INVALID, "sieve: removed_value = %d is not in 0 ... 255", removed_value);
    if (H < 1 || W < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "sieve: H = %d, W = %d: both must be at least 1", H, W);
    if ((int64_t)H * W > 0x7fffffff) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "sieve: more than 2^31 - 1 pixels");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t n = (int64_t)H * W;
    *n_removed = 0;
    if (min_area <= 1) {   // no component has fewer than one pixel: the identity
        HIPCHK(ctx, hipMemcpyAsync(d_out, d_q, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        return stream_sync(ctx);
    }
    RSCHK(ws_reserve(ctx, sizeof(int) * 2 * (size_t)n + 256));
    RSCHK(pin_reserve(ctx, 64));
    int *L = (int *)ctx->d_ws, *area = L + n;
    unsigned long long *d_cnt = (unsigned long long *)(ctx->d_ws + ((sizeof(int) * 2 * (size_t)n + 63) & ~(size_t)63));
    const unsigned g = k20_grid(n);
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), ctx->stream));
    {
        prof_scope ps(ctx, "sieve");
        hipLaunchKernelGGL(k20_cc_init, dim3(g), dim3(K20_THREADS), 0, ctx->stream, d_q, n, ignore, L, area);
        hipLaunchKernelGGL(k20_cc_union, dim3(g), dim3(K20_THREADS), 0, ctx->stream, d_q, H, W, ignore, connectivity == 8 ? 1 : 0, L);
        hipLaunchKernelGGL(k20_cc_count, dim3(g), dim3(K20_THREADS), 0, ctx->stream, n, L, area);
        hipLaunchKernelGGL(k20_cc_filter, dim3(g), dim3(K20_THREADS), 0, ctx->stream, d_q, n, (const int *)L, (const int *)area, min_area, removed_value, d_out,
                           d_cnt);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    *n_removed = (int64_t)((const unsigned long long *)ctx->h_pin)[0];
    return RSSEG_OK;
}
