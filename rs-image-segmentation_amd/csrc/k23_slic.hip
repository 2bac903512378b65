// K23 — SLIC superpixels on uint8 feature planes, and the per-segment reductions of object-based classification.  Neither
// has a counterpart in the reference; the semantics are this project's own (include/rsseg.h) and are restated in NumPy in
// tests/slic_ref.py, to which every result is equal bit for bit.
//
// Segmentation.  Centres sit on a grid of step S (ny x nx cells, id k = cy nx + cx); a pixel's candidates are the centres of
// the 3 x 3 cells around ITS cell, which never changes.  A centre is the float64 ratio of exact integer sums (count, sum y,
// sum x, sum q_p over its valid pixels), so it does not depend on the order the atomics land in; the distance is evaluated in
// float64, one IEEE operation per written operation, candidates in ascending id, the first strictly smaller one wins.
//   INVARIANT: a pixel's current label is always one of its nine candidates (it starts as its own cell and only ever moves
// to a candidate) and that centre is alive (the pixel itself is counted in it), so every valid pixel has a candidate.
//   k23_assign walks 64 x 16 tiles; a thread owns four consecutive pixels of a row.  The centres a tile can reach (its cells
// and one ring around them) are staged in LDS, and so are their accumulators, as 32-bit sums of tile-relative coordinates:
// a thread adds a RUN of pixels with the same winner at once, and the workgroup flushes the accumulators that were touched
// with 64-bit atomics.  The same kernel with INIT set writes the grid labels and their sums.
//   The host reads the changed count after every iteration (one wait each) and stops at the first zero.
//
// Connectivity.  4-connected components of equal centre id through the union-find of cc.h; components below min_area give up
// their pixels, which are grown over in Jacobi rounds (two planes; up, left, right, down; the first neighbour that was
// assigned when the round began).  K23_ROUNDS rounds are queued per host read: a round that assigns nothing copies its
// input, so the rounds queued behind it change nothing.
//   A plane entry is: root >= 0 (assigned), -1 (masked), -2 - root (valid, not assigned; root is its small component's).
// Final numbering: the smallest pixel index of every segment (atomicMin), a flag plane of those first pixels, the tile scan of
// K19 (rsseg_compact_plan) and a rank within the tile.
//
// Reductions.  segment_sums / segment_majority walk runs of eight consecutive pixels and commit a run of equal segment (and
// class) with one atomic per field; float32 planes are summed as to_fixed40 integers, exact for |x| < 2^11.
#include <algorithm>

#include "cc.h"
#include "keyed_table.h"

#define K23_ROUNDS 8     // growth rounds queued per host read
#define K23_RUN 8        // pixels per thread of the reductions
#define K23_SCAN_TILE 4096

extern "C" void rsseg_slic_tile(int *tw, int *th)
{
    if (tw) *tw = KT_TW;
    if (th) *th = KT_TH;
}

// grid-stride kernels: at most K23_MAX_BLOCKS workgroups, so that the one atomic a workgroup commits its counter with
// (wg_count_commit) stays rare (a million same-address atomics per launch cost more than the pass itself)
#define K23_MAX_BLOCKS 8192
static inline unsigned k23_grid(int64_t n) { return (unsigned)std::min<int64_t>(K23_MAX_BLOCKS, std::max<int64_t>(1, ceil_div64(n, KT_THREADS))); }

// ---- assignment + accumulation ---------------------------------------------------------------------------------------
// cen / acc: [K][F = P + 3] = {count, sum y, sum x, sum q_0 ...}; lcy x lcx: the local table of centres, whose entry (0, 0) is
// grid cell (ty0 / S - 1, tx0 / S - 1).  Dynamic LDS: double[nloc * F] (not with INIT), then unsigned[nloc * F].
template <int PMAX, bool INIT>
__global__ __launch_bounds__(KT_THREADS) void k23_assign(kt_planes_t pl, int P, const uint8_t *__restrict__ mask, int H, int W, int S, int ny, int nx,
                                                          int tiles_x, int lcy, int lcx, double weight, const double *__restrict__ cen,
                                                          int *__restrict__ lab, unsigned long long *__restrict__ acc, unsigned long long *__restrict__ changed)
{
    extern __shared__ __align__(8) unsigned char k23_lds[];
    const int F = P + 3, nloc = lcy * lcx, tid = threadIdx.x;
    double *s_cen = reinterpret_cast<double *>(k23_lds);
    unsigned *s_acc = reinterpret_cast<unsigned *>(k23_lds + (INIT ? (size_t)0 : (size_t)nloc * F * sizeof(double)));
    const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * KT_TW, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * KT_TH;
    const int gy0 = ty0 / S - 1, gx0 = tx0 / S - 1;
    for (int e = tid; e < nloc * F; e += KT_THREADS) {
        s_acc[e] = 0;
        if (!INIT) {
            const int li = e / F, f = e - li * F, gy = gy0 + li / lcx, gx = gx0 + li % lcx;
            const bool in = gy >= 0 && gy < ny && gx >= 0 && gx < nx;
            s_cen[e] = in ? cen[((int64_t)gy * nx + gx) * F + f] : 0.0;   // a cell outside the grid reads as a dead centre
        }
    }
    __syncthreads();
    const int ry = kt_ry(tid), y = ty0 + ry, xb = tx0 + kt_cx(tid);
    unsigned nchanged = 0, rc = 0, rx = 0, rq[PMAX];
    int run_li = -1;
#pragma unroll
    for (int p = 0; p < PMAX; p++) rq[p] = 0;
    auto flush = [&]() {
        if (run_li >= 0 && rc) {
            unsigned *a = s_acc + run_li * F;
            atomicAdd(a, rc);
            atomicAdd(a + 1, rc * (unsigned)ry);
            atomicAdd(a + 2, rx);
#pragma unroll
            for (int p = 0; p < PMAX; p++)
                if (p < P) atomicAdd(a + 3 + p, rq[p]);
        }
    };
    if (y < H) {
        const int cyp = y / S;
        for (int j = 0; j < KT_PXT; j++) {
            const int x = xb + j;
            if (x >= W) break;
            const int64_t i = (int64_t)y * W + x;
            const int cxp = x / S;
            int old;
            if (INIT) {
                old = (!mask || mask[i]) ? cyp * nx + cxp : -1;
                lab[i] = old;
            } else
                old = lab[i];
            if (old < 0) continue;
            unsigned qb[PMAX];
#pragma unroll
            for (int p = 0; p < PMAX; p++) qb[p] = p < P ? (unsigned)reinterpret_cast<const uint8_t *>(pl.p[p])[i] : 0u;
            int best = -1, best_li = -1;
            if (INIT) {
                best = old;
                best_li = (cyp - gy0) * lcx + (cxp - gx0);
            } else {
                double bestD = 0.0;
                for (int dy = -1; dy <= 1; dy++) {
                    const int gy = cyp + dy;
                    if (gy < 0 || gy >= ny) continue;
                    for (int dx = -1; dx <= 1; dx++) {
                        const int gx = cxp + dx;
                        if (gx < 0 || gx >= nx) continue;
                        const int li = (gy - gy0) * lcx + (gx - gx0);   // 0 <= gy - gy0 <= (TH - 1) / S + 3 < lcy, likewise in x
                        const double *c = s_cen + li * F;
                        if (c[0] == 0.0) continue;                      // dead: no pixel holds it
                        double dc = 0.0;
#pragma unroll
                        for (int p = 0; p < PMAX; p++)
                            if (p < P) {
                                const double d = (double)qb[p] - c[3 + p];
                                dc = dc + d * d;
                            }
                        const double ddy = (double)y - c[1], ddx = (double)x - c[2];
                        const double ds = ddy * ddy + ddx * ddx;
                        const double D = dc + weight * ds;
                        if (best < 0 || D < bestD) {                    // the first candidate, then strictly smaller only: ties keep the smaller id
                            bestD = D;
                            best = gy * nx + gx;
                            best_li = li;
                        }
                    }
                }
                // best >= 0 by the invariant above: the centre of `old` is a candidate and alive
                if (best != old) {
                    lab[i] = best;
                    nchanged++;
                }
            }
            if (best_li != run_li) {
                flush();
                run_li = best_li;
                rc = 0;
                rx = 0;
#pragma unroll
                for (int p = 0; p < PMAX; p++) rq[p] = 0;
            }
            rc++;
            rx += (unsigned)(x - tx0);
#pragma unroll
            for (int p = 0; p < PMAX; p++) rq[p] += qb[p];
        }
    }
    flush();
    __syncthreads();
    // a tile holds 1024 pixels: its 32-bit sums are at most 1024 * 255; the tile origin is added in 64 bits here
    for (int li = tid; li < nloc; li += KT_THREADS) {
        const unsigned c = s_acc[li * F];
        if (!c) continue;
        const int gy = gy0 + li / lcx, gx = gx0 + li % lcx;             // inside the grid: only such a centre can win
        unsigned long long *g = acc + ((int64_t)gy * nx + gx) * F;
        atomicAdd(g, (unsigned long long)c);
        atomicAdd(g + 1, (unsigned long long)s_acc[li * F + 1] + (unsigned long long)c * (unsigned)ty0);
        atomicAdd(g + 2, (unsigned long long)s_acc[li * F + 2] + (unsigned long long)c * (unsigned)tx0);
        for (int p = 0; p < P; p++) atomicAdd(g + 3 + p, (unsigned long long)s_acc[li * F + 3 + p]);
    }
    if (!INIT) wg_count_commit<KT_THREADS>(changed, nchanged);
}

// cen[k][0] = count, cen[k][f] = float64(sum) / float64(count): one IEEE division per component (0 for a dead centre)
__global__ __launch_bounds__(KT_THREADS) void k23_centres(const unsigned long long *__restrict__ acc, int64_t K, int F, double *__restrict__ cen)
{
    const int64_t total = K * F;
    for (int64_t e = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * KT_THREADS) {
        const int64_t k = e / F;
        const long long c = (long long)acc[k * F];
        const double cd = (double)c;
        cen[e] = e == k * F ? cd : (c ? (double)(long long)acc[e] / cd : 0.0);
    }
}

// ---- connectivity ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KT_THREADS) void k23_cc_init(const int *__restrict__ lab, int64_t n, int *__restrict__ L, int *__restrict__ area)
{
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        L[i] = lab[i] >= 0 ? (int)i : -1;
        area[i] = 0;
    }
}
__global__ __launch_bounds__(KT_THREADS) void k23_cc_union(const int *__restrict__ lab, int H, int W, int *__restrict__ L)
{
    const int64_t n = (int64_t)H * W;
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        const int v = lab[i];
        if (v < 0) continue;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        if (x > 0 && lab[i - 1] == v) cc_union(L, (int)i, (int)i - 1);
        if (y > 0 && lab[i - W] == v) cc_union(L, (int)i, (int)(i - W));
    }
}
// flattens the parents and counts the areas: a thread walks K23_RUN consecutive pixels and adds a run of one root at once
__global__ __launch_bounds__(KT_THREADS) void k23_cc_count(int64_t n, int *__restrict__ L, int *__restrict__ area)
{
    for (int64_t i0 = ((int64_t)blockIdx.x * KT_THREADS + threadIdx.x) * K23_RUN; i0 < n; i0 += (int64_t)gridDim.x * KT_THREADS * K23_RUN) {
        int cur = -1, run = 0;
        for (int j = 0; j < K23_RUN; j++) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            if (L[i] < 0) continue;
            const int r = cc_find(L, (int)i);
            L[i] = r;                  // roots never change after the union pass, so flattening here is safe
            if (r != cur) {
                if (run) atomicAdd(&area[cur], run);
                cur = r;
                run = 0;
            }
            run++;
        }
        if (run) atomicAdd(&area[cur], run);
    }
}
// A[i] = root (component of at least min_area pixels), -2 - root (a small one), -1 (masked); cnt[0] += pixels not assigned
__global__ __launch_bounds__(KT_THREADS) void k23_mark(int64_t n, const int *__restrict__ L, const int *__restrict__ area, int min_area, int *__restrict__ A,
                                                        unsigned long long *__restrict__ cnt)
{
    unsigned open = 0;
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        int a = -1;
        const int r = L[i];   // the root itself: k23_cc_count flattened every parent in a launch after the last union
        if (r >= 0) {
            const bool small = area[r] < min_area;
            a = small ? -2 - r : r;
            open += small;
        }
        A[i] = a;
    }
    wg_count_commit<KT_THREADS>(cnt, open);
}
// one Jacobi round: B = A, except that a pixel not assigned in A takes its first assigned neighbour (up, left, right, down)
__global__ __launch_bounds__(KT_THREADS) void k23_grow(const int *__restrict__ A, int *__restrict__ B, int H, int W, unsigned long long *__restrict__ cnt)
{
    const int64_t n = (int64_t)H * W;
    unsigned grown = 0;
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        int a = A[i];
        if (a <= -2) {
            const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
            int t;
            if (y > 0 && (t = A[i - W]) >= 0) a = t;
            else if (x > 0 && (t = A[i - 1]) >= 0) a = t;
            else if (x + 1 < W && (t = A[i + 1]) >= 0) a = t;
            else if (y + 1 < H && (t = A[i + W]) >= 0) a = t;
            grown += a >= 0;
        }
        B[i] = a;
    }
    wg_count_commit<KT_THREADS>(cnt, grown);
}

// the segment a pixel ends in.  A pixel still unassigned when the growth stops has no assigned neighbour; neither has any
// valid pixel 4-connected to it (it would have been assigned in an earlier round and this one in the next), so its small
// component, which is 4-connected, is unassigned as a whole and stays the segment it was.
__device__ __forceinline__ int k23_key(int a) { return a >= 0 ? a : (a <= -2 ? -2 - a : -1); }

__global__ __launch_bounds__(KT_THREADS) void k23_first(int64_t n, const int *__restrict__ A, unsigned *__restrict__ first)
{
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        const int k = k23_key(A[i]);
        if (k >= 0 && first[k] > (unsigned)i) atomicMin(&first[k], (unsigned)i);
    }
}
__global__ __launch_bounds__(KT_THREADS) void k23_flag(int64_t n, const int *__restrict__ A, const unsigned *__restrict__ first, uint8_t *__restrict__ flag)
{
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        const int k = k23_key(A[i]);
        flag[i] = k >= 0 && first[k] == (unsigned)i ? 1 : 0;
    }
}
// num[i] = 1 + the number of flagged pixels before i, for every flagged i; off: the exclusive tile sums of rsseg_compact_plan.
// One workgroup per tile of K23_SCAN_TILE pixels, 16 per thread.
__global__ __launch_bounds__(KT_THREADS) void k23_number(const uint8_t *__restrict__ flag, const int64_t *__restrict__ off, int64_t n, int *__restrict__ num)
{
    __shared__ int s_w[KT_THREADS / WAVE];
    const int64_t base = (int64_t)blockIdx.x * K23_SCAN_TILE + (int64_t)threadIdx.x * 16;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (base + j < n && flag[base + j]) m |= 1u << j;
    const int c = __popc(m);
    const int incl = wave_incl_scan(c);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 63) s_w[w] = incl;
    __syncthreads();
    int before = 0;
    for (int i = 0; i < w; i++) before += s_w[i];
    int r = (int)off[blockIdx.x] + before + incl - c;
#pragma unroll
    for (int j = 0; j < 16; j++)
        if ((m >> j) & 1u) num[base + j] = ++r;
}
__global__ __launch_bounds__(KT_THREADS) void k23_final(int64_t n, const int *__restrict__ A, const unsigned *__restrict__ first, const int *__restrict__ num,
                                                         int *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        const int k = k23_key(A[i]);
        out[i] = k >= 0 ? num[first[k]] : 0;
    }
}

// ---- reductions ------------------------------------------------------------------------------------------------------------
// sums[s][0 .. 3 + P) += {1, y, x, plane values} over the pixels of segment s (1 ... nseg) whose mask byte is non-zero
template <typename T>
__global__ __launch_bounds__(KT_THREADS) void k23_seg_sums(const int *__restrict__ seg, const uint8_t *__restrict__ mask, int64_t n, int W, int64_t nseg,
                                                            kt_planes_t pl, int P, unsigned long long *__restrict__ sums, unsigned long long *__restrict__ bad)
{
    const int F = P + 3;
    unsigned nbad = 0;
    for (int64_t i0 = ((int64_t)blockIdx.x * KT_THREADS + threadIdx.x) * K23_RUN; i0 < n; i0 += (int64_t)gridDim.x * KT_THREADS * K23_RUN) {
        int cur = 0;
        long long rc = 0, ry = 0, rx = 0, rq[KT_MAX_P];
#pragma unroll
        for (int p = 0; p < KT_MAX_P; p++) rq[p] = 0;
        auto flush = [&]() {
            if (cur > 0 && rc) {
                unsigned long long *g = sums + (int64_t)cur * F;
                atomicAdd(g, (unsigned long long)rc);
                atomicAdd(g + 1, (unsigned long long)ry);
                atomicAdd(g + 2, (unsigned long long)rx);
#pragma unroll
                for (int p = 0; p < KT_MAX_P; p++)
                    if (p < P) atomicAdd(g + 3 + p, (unsigned long long)rq[p]);
            }
        };
        for (int j = 0; j < K23_RUN; j++) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            const int s = seg[i];   // K25's rule for the effective label
            if (s < 0 || s > nseg) {
                nbad++;
                continue;
            }
            if (s == 0 || (mask && !mask[i])) continue;
            if (s != cur) {
                flush();
                cur = s;
                rc = ry = rx = 0;
#pragma unroll
                for (int p = 0; p < KT_MAX_P; p++) rq[p] = 0;
            }
            const int64_t y = i / W;
            rc++;
            ry += y;
            rx += i - y * W;
#pragma unroll
            for (int p = 0; p < KT_MAX_P; p++)
                if (p < P) {
                    const T v = reinterpret_cast<const T *>(pl.p[p])[i];
                    if constexpr (sizeof(T) == 1) rq[p] += (long long)v;
                    else rq[p] += to_fixed40((double)v);
                }
        }
        flush();
    }
    wg_count_commit<KT_THREADS>(bad, nbad);
}

// votes[(s - 1) * NL + v] += 1 for every pixel of segment s whose class v is below NL and not `ignore`
__global__ __launch_bounds__(KT_THREADS) void k23_seg_votes(const int *__restrict__ seg, const uint8_t *__restrict__ q, int64_t n, int64_t nseg, int NL,
                                                             int ignore, int *__restrict__ votes, unsigned long long *__restrict__ bad)
{
    unsigned nbad = 0;
    for (int64_t i0 = ((int64_t)blockIdx.x * KT_THREADS + threadIdx.x) * K23_RUN; i0 < n; i0 += (int64_t)gridDim.x * KT_THREADS * K23_RUN) {
        int64_t cur = -1;
        int run = 0;
        for (int j = 0; j < K23_RUN; j++) {
            const int64_t i = i0 + j;
            if (i >= n) break;
            const int s = seg[i];
            if (s < 0 || s > nseg) {
                nbad++;
                continue;
            }
            const int v = q[i];
            if (s == 0 || v == ignore || v >= NL) continue;
            const int64_t cell = (int64_t)(s - 1) * NL + v;
            if (cell != cur) {
                if (run) atomicAdd(&votes[cur], run);
                cur = cell;
                run = 0;
            }
            run++;
        }
        if (run) atomicAdd(&votes[cur], run);
    }
    wg_count_commit<KT_THREADS>(bad, nbad);
}
// table[s] = the label with the most votes (ties: the smallest), `fill` without a voter; table[0] = fill
__global__ __launch_bounds__(KT_THREADS) void k23_seg_winner(const int *__restrict__ votes, int64_t nseg, int NL, int fill, uint8_t *__restrict__ table)
{
    for (int64_t s = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; s <= nseg; s += (int64_t)gridDim.x * KT_THREADS) {
        int win = fill, most = 0;
        if (s > 0) {
            const int *row = votes + (s - 1) * NL;
            for (int v = 0; v < NL; v++) {
                const int c = row[v];
                if (c > most) {
                    most = c;
                    win = v;
                }
            }
        }
        table[s] = (uint8_t)win;
    }
}
template <typename T>
__global__ __launch_bounds__(KT_THREADS) void k23_paint(const int *__restrict__ seg, int64_t n, int64_t nseg, const T *__restrict__ table, T *__restrict__ out,
                                                         unsigned long long *__restrict__ bad)
{
    unsigned nbad = 0;
    for (int64_t i = (int64_t)blockIdx.x * KT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KT_THREADS) {
        const int s = seg[i];
        const bool ok = s >= 0 && s <= nseg;
        out[i] = table[ok ? s : 0];
        nbad += !ok;
    }
    wg_count_commit<KT_THREADS>(bad, nbad);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
namespace {

size_t k23_up(size_t b) { return (b + 255) & ~(size_t)255; }

template <bool INIT>
int k23_launch_assign(rsseg_ctx *ctx, const kt_planes_t &pl, int P, const uint8_t *d_mask, int H, int W, int S, int ny, int nx, double weight,
                      const double *cen, int *lab, unsigned long long *acc, unsigned long long *changed)
{
    const int tiles_x = (W + KT_TW - 1) / KT_TW, tiles_y = (H + KT_TH - 1) / KT_TH;
    const int lcy = (KT_TH - 1) / S + 4, lcx = (KT_TW - 1) / S + 4;
    const size_t lds = (size_t)lcy * lcx * (P + 3) * (INIT ? sizeof(unsigned) : sizeof(unsigned) + sizeof(double));
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y)), block(KT_THREADS);
    const auto kernel = P <= 4 ? k23_assign<4, INIT> : P <= 8 ? k23_assign<8, INIT> : k23_assign<16, INIT>;
    RSCHK(kt_launch(ctx, kernel, grid, block, lds, pl, P, d_mask, H, W, S, ny, nx, tiles_x, lcy, lcx, weight, cen, lab, acc, changed));
    HIPCHK(ctx, hipGetLastError());
    return RSSEG_OK;
}

// the flat segment map of the reductions: a segment holds a pixel, so there are at most n of them (the pointer is tested first)
int k23_check_seg(rsseg_ctx *ctx, const char *what, const int32_t *d_seg, int64_t n, int64_t n_segments)
{
    RSCHK(kt_check_seg(ctx, what, d_seg));
    RSCHK(kt_check_pixels(ctx, what, n));
    return kt_check_nseg(ctx, what, n_segments, n, nullptr);
}

int k23_bad_labels(rsseg_ctx *ctx, const char *what, const unsigned long long *d_bad, int64_t n_segments)
{
    unsigned long long bad = 0;
    RSCHK(kt_read(ctx, d_bad, sizeof(bad), &bad));
    return kt_bad_labels(ctx, what, bad, n_segments);
}

}  // namespace

extern "C" int rsseg_slic_u8(rsseg_ctx *ctx, const uint8_t *const *d_planes, int P, int H, int W, const uint8_t *d_mask, int S, double weight, int max_iter,
                             int min_area, int32_t *d_labels, int64_t *n_segments, int *n_iter, int64_t *n_regrown)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: d_planes is null");
    RSCHK(kt_check_planes(ctx, "slic", d_planes, P, 1));
    for (int p = 0; p < P; p++) RSCHK(kt_check_plane_u8(ctx, "slic", d_planes, p));
    RSCHK(kt_check_hw(ctx, "slic", H, W));
    if ((int64_t)H * W > 0x7fffffff) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "slic: more than 2^31 - 1 pixels");
    if (S < 2 || S > 4096) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: S = %d is not in 2 ... 4096", S);
    if (!(weight >= 0.0) || !std::isfinite(weight)) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: weight = %g is not a finite non-negative number", weight);
    if (max_iter < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: max_iter = %d is negative", max_iter);
    if (min_area < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: min_area = %d is negative", min_area);
    if (!d_labels || ((uintptr_t)d_labels & 3)) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: d_labels null or not aligned to its element");
    if (!n_segments) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: n_segments is null");
    if (!n_iter) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: n_iter is null");
    if (!n_regrown) return rs_fail(ctx, RSSEG_ERR_INVALID, "slic: n_regrown is null");
    if (rsseg_compact_tile() != K23_SCAN_TILE) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "slic: the scan tile of K19 is not %d pixels", K23_SCAN_TILE);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t n = (int64_t)H * W;
    const int ny = (H + S - 1) / S, nx = (W + S - 1) / S, F = P + 3;
    const int64_t K = (int64_t)ny * nx, ntiles = ceil_div64(n, K23_SCAN_TILE);
    // workspace: four int planes, the flag plane, the tile offsets, accumulators, centres, counters
    const size_t b_plane = k23_up(sizeof(int) * (size_t)n), b_flag = k23_up((size_t)n), b_off = k23_up(sizeof(int64_t) * (size_t)(ntiles + 1));
    const size_t b_acc = k23_up(sizeof(unsigned long long) * (size_t)K * F), b_cnt = k23_up(sizeof(unsigned long long) * (K23_ROUNDS + 2));
    RSCHK(ws_reserve(ctx, 4 * b_plane + b_flag + b_off + 2 * b_acc + b_cnt));
    RSCHK(pin_reserve(ctx, 256));
    char *w = ctx->d_ws;
    int *Lp = (int *)w, *area = (int *)(w + b_plane), *A = (int *)(w + 2 * b_plane), *B = (int *)(w + 3 * b_plane);
    w += 4 * b_plane;
    uint8_t *flag = (uint8_t *)w;
    w += b_flag;
    int64_t *off = (int64_t *)w;
    w += b_off;
    unsigned long long *acc = (unsigned long long *)w;
    w += b_acc;
    double *cen = (double *)w;
    w += b_acc;
    unsigned long long *cnt = (unsigned long long *)w;
    kt_planes_t pl;
    memset(&pl, 0, sizeof(pl));
    for (int p = 0; p < P; p++) pl.p[p] = d_planes[p];
    int *lab = d_labels;
    const unsigned g = k23_grid(n);

    // ---- iterations ----
    int iters = 0;
    {
        prof_scope ps(ctx, "slic_init");
        HIPCHK(ctx, hipMemsetAsync(acc, 0, sizeof(unsigned long long) * (size_t)K * F, ctx->stream));
        RSCHK(k23_launch_assign<true>(ctx, pl, P, d_mask, H, W, S, ny, nx, weight, nullptr, lab, acc, nullptr));
    }
    for (int t = 1; t <= max_iter; t++) {
        {
            prof_scope ps(ctx, "slic_assign");
            hipLaunchKernelGGL(k23_centres, dim3(k23_grid(K * F)), dim3(KT_THREADS), 0, ctx->stream, (const unsigned long long *)acc, K, F, cen);
            HIPCHK(ctx, hipMemsetAsync(acc, 0, sizeof(unsigned long long) * (size_t)K * F, ctx->stream));
            HIPCHK(ctx, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), ctx->stream));
            RSCHK(k23_launch_assign<false>(ctx, pl, P, nullptr, H, W, S, ny, nx, weight, cen, lab, acc, cnt));
        }
        unsigned long long changed = 0;
        RSCHK(kt_read(ctx, cnt, sizeof(changed), &changed));
        iters = t;
        if (!changed) break;
    }

    // ---- connectivity ----
    unsigned long long regrown = 0;
    int *cur = A, *other = B;
    {
        prof_scope ps(ctx, "slic_enforce");
        HIPCHK(ctx, hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * (K23_ROUNDS + 2), ctx->stream));
        hipLaunchKernelGGL(k23_cc_init, dim3(g), dim3(KT_THREADS), 0, ctx->stream, (const int *)lab, n, Lp, area);
        hipLaunchKernelGGL(k23_cc_union, dim3(g), dim3(KT_THREADS), 0, ctx->stream, (const int *)lab, H, W, Lp);
        hipLaunchKernelGGL(k23_cc_count, dim3(k23_grid(ceil_div64(n, K23_RUN))), dim3(KT_THREADS), 0, ctx->stream, n, Lp, area);
        hipLaunchKernelGGL(k23_mark, dim3(g), dim3(KT_THREADS), 0, ctx->stream, n, (const int *)Lp, (const int *)area, min_area, A, cnt);
        HIPCHK(ctx, hipGetLastError());
    }
    unsigned long long open = 0;
    RSCHK(kt_read(ctx, cnt, sizeof(open), &open));
    while (open) {
        unsigned long long got[K23_ROUNDS];
        {
            prof_scope ps(ctx, "slic_enforce");
            HIPCHK(ctx, hipMemsetAsync(cnt + 1, 0, sizeof(unsigned long long) * K23_ROUNDS, ctx->stream));
            for (int r = 0; r < K23_ROUNDS; r++) {
                hipLaunchKernelGGL(k23_grow, dim3(g), dim3(KT_THREADS), 0, ctx->stream, (const int *)cur, other, H, W, cnt + 1 + r);
                std::swap(cur, other);
            }
            HIPCHK(ctx, hipGetLastError());
        }
        RSCHK(kt_read(ctx, cnt + 1, sizeof(got), got));
        bool stopped = false;
        for (int r = 0; r < K23_ROUNDS; r++) {
            regrown += got[r];
            stopped = stopped || got[r] == 0;
        }
        if (stopped) break;
    }

    // ---- numbering ----
    unsigned *first = (unsigned *)Lp;   // the parents and the areas are no longer needed
    int *num = area;
    {
        prof_scope ps(ctx, "slic_relabel");
        HIPCHK(ctx, hipMemsetAsync(first, 0xff, sizeof(unsigned) * (size_t)n, ctx->stream));
        hipLaunchKernelGGL(k23_first, dim3(g), dim3(KT_THREADS), 0, ctx->stream, n, (const int *)cur, first);
        hipLaunchKernelGGL(k23_flag, dim3(g), dim3(KT_THREADS), 0, ctx->stream, n, (const int *)cur, (const unsigned *)first, flag);
        HIPCHK(ctx, hipGetLastError());
    }
    int64_t nseg = 0;
    RSCHK(rsseg_compact_plan(ctx, flag, n, off, &nseg));
    {
        prof_scope ps(ctx, "slic_relabel");
        hipLaunchKernelGGL(k23_number, dim3((unsigned)ntiles), dim3(KT_THREADS), 0, ctx->stream, (const uint8_t *)flag, (const int64_t *)off, n, num);
        hipLaunchKernelGGL(k23_final, dim3(g), dim3(KT_THREADS), 0, ctx->stream, n, (const int *)cur, (const unsigned *)first, (const int *)num, d_labels);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, rs_sync(ctx));
    *n_segments = nseg;
    *n_iter = iters;
    *n_regrown = (int64_t)regrown;
    return RSSEG_OK;
}

extern "C" int rsseg_segment_sums(rsseg_ctx *ctx, const int32_t *d_seg, int H, int W, int64_t n_segments, const void *const *d_planes, int P, int dtype,
                                  const uint8_t *d_mask, int64_t *d_sums)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    RSCHK(kt_check_hw(ctx, "segment_sums", H, W));
    const int64_t n = (int64_t)H * W;
    RSCHK(k23_check_seg(ctx, "segment_sums", d_seg, n, n_segments));
    RSCHK(kt_check_planes(ctx, "segment_sums", d_planes, P, 0));
    RSCHK(kt_check_dtype(ctx, "segment_sums", dtype, "RSSEG_U8 or RSSEG_F32"));
    for (int p = 0; p < P; p++) RSCHK(kt_check_plane(ctx, "segment_sums", d_planes, p, dtype));
    if (!d_sums || ((uintptr_t)d_sums & 7)) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_sums: d_sums null or not 8-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RSCHK(ws_reserve(ctx, 256));
    RSCHK(pin_reserve(ctx, 256));
    unsigned long long *d_bad = (unsigned long long *)ctx->d_ws;
    kt_planes_t pl;
    memset(&pl, 0, sizeof(pl));
    for (int p = 0; p < P; p++) pl.p[p] = d_planes[p];
    HIPCHK(ctx, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(d_sums, 0, sizeof(int64_t) * (size_t)(n_segments + 1) * (P + 3), ctx->stream));
    {
        prof_scope ps(ctx, "segment_sums");
        const unsigned g = k23_grid(ceil_div64(n, K23_RUN));
        if (dtype == RSSEG_U8)
            hipLaunchKernelGGL(k23_seg_sums<uint8_t>, dim3(g), dim3(KT_THREADS), 0, ctx->stream, d_seg, d_mask, n, W, n_segments, pl, P,
                               (unsigned long long *)d_sums, d_bad);
        else
            hipLaunchKernelGGL(k23_seg_sums<float>, dim3(g), dim3(KT_THREADS), 0, ctx->stream, d_seg, d_mask, n, W, n_segments, pl, P,
                               (unsigned long long *)d_sums, d_bad);
        HIPCHK(ctx, hipGetLastError());
    }
    return k23_bad_labels(ctx, "segment_sums", d_bad, n_segments);
}

extern "C" int rsseg_segment_majority_u8(rsseg_ctx *ctx, const int32_t *d_seg, int64_t n, int64_t n_segments, const uint8_t *d_class, int ignore, int fill,
                                         uint8_t *d_table)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    RSCHK(k23_check_seg(ctx, "segment_majority", d_seg, n, n_segments));
    if (!d_class) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_majority: d_class is null");
    if (!d_table) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_majority: d_table is null");
    if (ignore < -1 || ignore > 255) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_majority: ignore = %d is neither -1 (none) nor a value in 0 ... 255", ignore);
    if (fill < 0 || fill > 255) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_majority: fill = %d is not in 0 ... 255", fill);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the largest label that votes decides the width of the table
    int64_t counts[256];
    RSCHK(rsseg_hist_u8(ctx, d_class, n, counts));
    int NL = 1;
    for (int v = 0; v < 256; v++)
        if (counts[v] && v != ignore) NL = v + 1;
    const int64_t cells = std::max<int64_t>(1, n_segments) * NL;
    if (cells * (int64_t)sizeof(int) > ((int64_t)1 << 31))
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "segment_majority: %lld segments x %d labels need a vote table above 2 GiB", (long long)n_segments, NL);
    const size_t b_votes = k23_up(sizeof(int) * (size_t)cells);
    RSCHK(ws_reserve(ctx, b_votes + 256));
    RSCHK(pin_reserve(ctx, 256));
    int *votes = (int *)ctx->d_ws;
    unsigned long long *d_bad = (unsigned long long *)(ctx->d_ws + b_votes);
    HIPCHK(ctx, hipMemsetAsync(votes, 0, b_votes + 256, ctx->stream));
    {
        prof_scope ps(ctx, "segment_majority");
        hipLaunchKernelGGL(k23_seg_votes, dim3(k23_grid(ceil_div64(n, K23_RUN))), dim3(KT_THREADS), 0, ctx->stream, d_seg, d_class, n, n_segments, NL, ignore,
                           votes, d_bad);
        hipLaunchKernelGGL(k23_seg_winner, dim3(k23_grid(n_segments + 1)), dim3(KT_THREADS), 0, ctx->stream, (const int *)votes, n_segments, NL, fill,
                           d_table);
        HIPCHK(ctx, hipGetLastError());
    }
    return k23_bad_labels(ctx, "segment_majority", d_bad, n_segments);
}

extern "C" int rsseg_segment_paint(rsseg_ctx *ctx, const int32_t *d_seg, int64_t n, int64_t n_segments, const void *d_table, int elem_bytes, void *d_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    RSCHK(k23_check_seg(ctx, "segment_paint", d_seg, n, n_segments));
    if (elem_bytes != 1 && elem_bytes != 4) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_paint: elem_bytes = %d, must be 1 or 4", elem_bytes);
    if (!d_table || ((uintptr_t)d_table & (elem_bytes - 1))) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_paint: d_table null or not aligned to its element");
    if (!d_out || ((uintptr_t)d_out & (elem_bytes - 1))) return rs_fail(ctx, RSSEG_ERR_INVALID, "segment_paint: d_out null or not aligned to its element");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RSCHK(ws_reserve(ctx, 256));
    RSCHK(pin_reserve(ctx, 256));
    unsigned long long *d_bad = (unsigned long long *)ctx->d_ws;
    HIPCHK(ctx, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), ctx->stream));
    {
        prof_scope ps(ctx, "segment_paint");
        if (elem_bytes == 1)
            hipLaunchKernelGGL(k23_paint<uint8_t>, dim3(k23_grid(n)), dim3(KT_THREADS), 0, ctx->stream, d_seg, n, n_segments, (const uint8_t *)d_table,
                               (uint8_t *)d_out, d_bad);
        else
            hipLaunchKernelGGL(k23_paint<uint32_t>, dim3(k23_grid(n)), dim3(KT_THREADS), 0, ctx->stream, d_seg, n, n_segments, (const uint32_t *)d_table,
                               (uint32_t *)d_out, d_bad);
        HIPCHK(ctx, hipGetLastError());
    }
    return k23_bad_labels(ctx, "segment_paint", d_bad, n_segments);
}
