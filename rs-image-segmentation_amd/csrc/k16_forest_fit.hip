// K16: random-forest training — scikit-learn 1.7.2's depth-first Gini best-split builder (tree/_tree.pyx:141-333,
// tree/_splitter.pyx:269-545), bootstrap weights as integer counts.  One workgroup owns one tree: its xorshift state,
// its `features` / `constant_features` permutations and an explicit DFS stack live in global memory between launches,
// and the whole workgroup works on one node at a time.  Node k+1's feature draws depend on everything nodes 0..k did
// (item 5 of the parity contract), so a tree is built strictly in sklearn's node order; trees run side by side.
//
// Per drawn feature the node's samples are gathered as 64-bit keys (order-preserving float32 bits << 32 | sample index),
// sorted (bitonic in LDS up to FF_LDS_SORT keys; above that LDS-sorted runs merged in global memory by rank: every key is
// unique, so each key's output slot is its run rank plus a binary search in the partner run), then scanned in chunks of
// 256 positions: per class an inclusive wave scan of the weights gives the left counts, the Gini proxy of every candidate
// position is evaluated in double, and the first maximum wins (strict > across positions and across features, as the
// splitter updates best_split).  Counts are integers (bootstrap weights), so every double sklearn forms from them is
// formed here from the same exact integers: sums of squares stay below 2^53 while the total weight is below 2^26.
//
// Bounds: a tree has at most 2m-1 nodes and its stack at most min(max_depth, m)+1 entries (m = samples with a non-zero
// count); the host sizes both exactly and the kernel still checks them (err, never a truncated tree).  A launch builds at most
// `budget` nodes per tree; the host issues continuation launches and stops when one makes no progress.
//
// Each tree is a job (rsseg_forest_job): its own count row, weight_total, seed, max_depth, min_samples_split,
// min_samples_leaf and max_features, read from device memory once per launch into SGPRs (uniform per workgroup).  A count
// row has length n and sums to the job's weight_total, which is the tree's weighted_n_samples; k16_fit_init refuses a row
// that does not (err 5).  Samples with count 0 never enter a tree (sklearn's splitter drops them too), so a row that is zero
// on the held-out samples of a cross-validation fold grows the tree of the fit on the fold's training subset, and trees of
// different folds, depths and forests share one launch chain.  rsseg_forest_fit is the uniform case: weight_total = n.
#include <cfloat>

#include "common.h"

#define FF_THREADS 256
#define FF_WAVES (FF_THREADS / 64)
#define FF_LDS_SORT 4096
#define FF_MAX_F 64
#define FF_MAX_C 64

namespace {

struct ff_state {
    int node_count, stack_size, max_depth_seen, done, err;
    uint32_t rng;
    int features[FF_MAX_F];
    int constants[FF_MAX_F];
};

struct ff_entry {
    int start, end, depth, parent, is_left, n_const;
    double impurity;
};

struct ff_args {
    const float *const *planes;   // F device pointers (device array)
    const int32_t *y;         // class index per sample
    const int32_t *counts;    // count rows of n values; tree t reads row jobs[t].counts_row
    const rsseg_forest_job *jobs;   // [T] per-tree parameters
    int64_t n;                // samples
    int F, C, T;
    int budget;
    const int64_t *samp_off;  // [T+1] samples / sort scratch of tree t
    const int64_t *node_off;  // [T+1] node records of tree t (2m-1 each)
    const int64_t *stack_off; // [T+1] stack entries of tree t
    int32_t *samples;
    uint64_t *g0, *g1;
    ff_state *st;
    ff_entry *stack;
    int32_t *left, *right, *feature, *n_node, *w_node;
    double *threshold, *impurity, *value;
    uint8_t *missing_left;
};

__device__ __forceinline__ uint32_t ff_key(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ff_val(uint64_t e)
{
    const uint32_t k = (uint32_t)(e >> 32);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// sklearn's our_rand_r (utils/_random.pxd:20-34) and rand_int (tree/_utils.pyx:55)
__device__ __forceinline__ uint32_t ff_rand(uint32_t *s)
{
    if (*s == 0) *s = 1u;
    *s ^= *s << 13;
    *s ^= *s >> 17;
    *s ^= *s << 5;
    return *s % (2147483647u + 1u);
}
__device__ __forceinline__ int ff_rand_int(int lo, int hi, uint32_t *s) { return lo + (int)(ff_rand(s) % (uint32_t)(hi - lo)); }

// "the same value" for the constant-feature test and next_p (b >= a in sorted order): `b <= a + FEATURE_THRESHOLD`.  The
// source declares FEATURE_THRESHOLD = 1e-7 in tree/_partitioner.pxd:13, but the released 1.7.2 build compares with 0: it
// splits two samples one float32 ulp apart at 0.5 (6e-8) or 2/255 +- 1e-7 (tests/test_forest_fit_host.py pins this against
// scikit-learn itself).  So values are the same only when equal.
__device__ __forceinline__ bool ff_close(float a, float b) { return b <= a; }

__device__ __forceinline__ int ff_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// exclusive prefix of `flag` over the workgroup; returns the prefix, *total = the count (all threads)
__device__ __forceinline__ int block_excl_count(int flag, int *s_w, int *total)
{
    const int w = threadIdx.x >> 6;
    const int inc = wave_incl_scan(flag);
    if (lane_id() == 63) s_w[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < FF_WAVES; i++) {
        if (i < w) off += s_w[i];
        tot += s_w[i];
    }
    __syncthreads();
    *total = tot;
    return off + inc - flag;
}

__device__ void bitonic_lds(uint64_t *buf, int P)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += FF_THREADS) {
                const int i = 2 * t - (t & (j - 1));
                const int l = i + j;
                const bool asc = (i & k) == 0;
                const uint64_t a = buf[i], b = buf[l];
                if ((a > b) == asc) {
                    buf[i] = b;
                    buf[l] = a;
                }
            }
            __syncthreads();
        }
}

struct ff_best {
    double score, gl, gr;
    int pos, wl;
};

__device__ __forceinline__ bool ff_better(const ff_best &a, const ff_best &b)   // a wins over b: higher score, then earlier position
{
    return a.score > b.score || (a.score == b.score && a.pos < b.pos);
}

struct ff_shared {
    uint64_t sortbuf[FF_LDS_SORT];
    int tot[FF_MAX_C];
    int base[FF_MAX_C];
    int wtot[FF_WAVES][FF_MAX_C];
    int s_w[FF_WAVES];
    ff_best red[FF_THREADS / 64];
    int features[FF_MAX_F], constants[FF_MAX_F];
    // node and draw state (written by thread 0)
    ff_entry cur;
    int action, fcur, fj, f_i, nvis, nfound, ndrawn, ntotal, nknown;
    int is_const;
    int wsum;
    long long sq;
    ff_best best;
    int best_feature;
    float b_lo, b_hi;
    uint32_t rng;
    int node_count, stack_size, max_depth_seen, err;
};

// sorted keys of the node's samples for plane f: LDS when n <= FF_LDS_SORT, otherwise g0 or g1 (returned)
__device__ const uint64_t *ff_sort(const ff_args &a, ff_shared &S, const int32_t *smp, int n, const float *plane, uint64_t *g0, uint64_t *g1)
{
    if (n <= FF_LDS_SORT) {
        int P = 2;
        while (P < n) P <<= 1;
        for (int i = threadIdx.x; i < P; i += FF_THREADS) {
            uint64_t e = ~0ull;
            if (i < n) {
                const int s = smp[i];
                e = ((uint64_t)ff_key(plane[s]) << 32) | (uint32_t)s;
            }
            S.sortbuf[i] = e;
        }
        __syncthreads();
        bitonic_lds(S.sortbuf, P);
        return S.sortbuf;
    }
    // runs of FF_LDS_SORT keys sorted in LDS
    for (int r0 = 0; r0 < n; r0 += FF_LDS_SORT) {
        const int len = min(FF_LDS_SORT, n - r0);
        for (int i = threadIdx.x; i < FF_LDS_SORT; i += FF_THREADS) {
            uint64_t e = ~0ull;
            if (i < len) {
                const int s = smp[r0 + i];
                e = ((uint64_t)ff_key(plane[s]) << 32) | (uint32_t)s;
            }
            S.sortbuf[i] = e;
        }
        __syncthreads();
        bitonic_lds(S.sortbuf, FF_LDS_SORT);
        for (int i = threadIdx.x; i < len; i += FF_THREADS) g0[r0 + i] = S.sortbuf[i];
        __syncthreads();
    }
    // merge pairs of runs by rank (keys are unique: the sample index is part of the key)
    uint64_t *src = g0, *dst = g1;
    for (int r = FF_LDS_SORT; r < n; r <<= 1) {
        for (int i = threadIdx.x; i < n; i += FF_THREADS) {
            const int lo = (i / (2 * r)) * (2 * r);
            const int mid = min(lo + r, n), hi = min(lo + 2 * r, n);
            const uint64_t e = src[i];
            int o;
            if (i < mid) {   // in run A: count B keys below e
                int l = mid, h = hi;
                while (l < h) {
                    const int m = (l + h) >> 1;
                    if (src[m] < e) l = m + 1;
                    else h = m;
                }
                o = lo + (i - lo) + (l - mid);
            } else {         // in run B: count A keys below e
                int l = lo, h = mid;
                while (l < h) {
                    const int m = (l + h) >> 1;
                    if (src[m] < e) l = m + 1;
                    else h = m;
                }
                o = lo + (i - mid) + (l - lo);
            }
            dst[o] = e;
        }
        __threadfence_block();
        __syncthreads();
        uint64_t *t = src;
        src = dst;
        dst = t;
    }
    return src;
}

// the best position of one feature over sorted keys `buf` (n of them): first maximum of the Gini proxy
__device__ ff_best ff_scan(const ff_args &a, ff_shared &S, const uint64_t *buf, int n, const int32_t *cnt, long long W, int msl)
{
    const int C = a.C, tid = threadIdx.x, w = tid >> 6;
    if (tid < C) S.base[tid] = 0;
    __syncthreads();
    ff_best best;
    best.score = -INFINITY;
    best.pos = 0x7fffffff;
    best.gl = best.gr = 0.0;
    best.wl = 0;
    for (int c0 = 0; c0 < n; c0 += FF_THREADS) {
        const int i = c0 + tid;
        const bool in = i < n;
        int cls = -1, wt = 0;
        bool cand = false;
        if (in) {
            const uint64_t e = buf[i];
            const int s = (int)(uint32_t)e;
            cls = a.y[s];
            wt = cnt[s];
            if (i + 1 < n) {
                const float v = ff_val(e), vn = ff_val(buf[i + 1]);
                cand = !ff_close(v, vn) && (i + 1) >= msl && (n - i - 1) >= msl;
            }
        }
        for (int c = 0; c < C; c++) {
            const int t = wave_sum(cls == c ? wt : 0);
            if (lane_id() == 0) S.wtot[w][c] = t;
        }
        __syncthreads();
        long long sqL = 0, sqR = 0;
        long long WL = 0;
        for (int c = 0; c < C; c++) {
            int off = S.base[c];
            for (int q = 0; q < w; q++) off += S.wtot[q][c];
            const long long L = (long long)off + wave_incl_scan(cls == c ? wt : 0);
            const long long R = (long long)S.tot[c] - L;
            sqL += L * L;
            sqR += R * R;
            WL += L;
        }
        if (cand) {
            const double wl = (double)WL, wr = (double)(W - WL);
            const double gl = 1.0 - (double)sqL / (wl * wl);
            const double gr = 1.0 - (double)sqR / (wr * wr);
            const double proxy = -wr * gr - wl * gl;
            if (proxy > best.score) {
                best.score = proxy;
                best.pos = i + 1;
                best.gl = gl;
                best.gr = gr;
                best.wl = (int)WL;
            }
        }
        __syncthreads();
        if (tid < C) {
            int s = 0;
            for (int q = 0; q < FF_WAVES; q++) s += S.wtot[q][tid];
            S.base[tid] += s;
        }
        __syncthreads();
    }
    // workgroup first-maximum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ff_best b;
        b.score = __shfl_xor(best.score, o, 64);
        b.gl = __shfl_xor(best.gl, o, 64);
        b.gr = __shfl_xor(best.gr, o, 64);
        b.pos = __shfl_xor(best.pos, o, 64);
        b.wl = __shfl_xor(best.wl, o, 64);
        if (ff_better(b, best)) best = b;
    }
    if (lane_id() == 0) S.red[w] = best;
    __syncthreads();
    best = S.red[0];
    for (int q = 1; q < FF_WAVES; q++)
        if (ff_better(S.red[q], best)) best = S.red[q];
    __syncthreads();
    return best;
}

__global__ void __launch_bounds__(FF_THREADS) k16_fit_init(const ff_args *__restrict__ pa)
{
    const ff_args &a = *pa;
    __shared__ int s_w[FF_WAVES];
    __shared__ int s_base;
    __shared__ int s_neg;
    __shared__ unsigned long long s_sum;
    const int t = blockIdx.x;
    if (t >= a.T) return;
    const int32_t *cnt = a.counts + a.jobs[t].counts_row * a.n;
    const int64_t weight_total = a.jobs[t].weight_total;
    int32_t *smp = a.samples + a.samp_off[t];
    const int64_t m = a.samp_off[t + 1] - a.samp_off[t];
    if (threadIdx.x == 0) {
        s_base = 0;
        s_neg = 0;
        s_sum = 0ull;
    }
    __syncthreads();
    long long wsum = 0;   // this thread's share of the row's total weight
    int neg = 0;
    for (int64_t c0 = 0; c0 < a.n; c0 += FF_THREADS) {
        const int64_t i = c0 + threadIdx.x;
        const int32_t ci = i < a.n ? cnt[i] : 0;
        const int flag = ci > 0 ? 1 : 0;
        wsum += ci;
        neg |= ci < 0;
        int tot;
        const int off = block_excl_count(flag, s_w, &tot);
        const int64_t o = (int64_t)s_base + off;
        if (flag && o < m) smp[o] = (int32_t)i;
        __syncthreads();
        if (threadIdx.x == 0) s_base += tot;
        __syncthreads();
    }
    // weighted_n_samples is the job's weight_total (k16_fit_step: w_total), so a count row must be non-negative and sum to it
    wsum = wave_sum(wsum);
    neg = wave_sum(neg);
    if (lane_id() == 0) {
        atomicAdd(&s_sum, (unsigned long long)wsum);
        if (neg) atomicOr(&s_neg, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ff_state *st = a.st + t;
        st->err = (s_neg || (long long)s_sum != (long long)weight_total) ? 5 : s_base != m ? 1 : 0;
        st->node_count = 0;
        st->max_depth_seen = 0;
        st->rng = a.jobs[t].seed;
        for (int f = 0; f < FF_MAX_F; f++) st->features[f] = st->constants[f] = f;
        ff_entry root;
        root.start = 0;
        root.end = (int)m;
        root.depth = 0;
        root.parent = -1;
        root.is_left = 0;
        root.n_const = 0;
        root.impurity = -1.0;   // computed from the root's counts (node_impurity)
        a.stack[a.stack_off[t]] = root;
        st->stack_size = 1;
        st->done = (m == 0 || st->err) ? 1 : 0;
    }
}

enum { FF_STOP = 0, FF_SKIP = 1, FF_EVAL = 2 };

__global__ void __launch_bounds__(FF_THREADS) k16_fit_step(const ff_args *__restrict__ pa)
{
    const ff_args &a = *pa;
    __shared__ ff_shared S;
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= a.T) return;
    ff_state *st = a.st + t;
    if (st->done) return;
    // the tree's own parameters, loaded once per launch.  They are uniform over the workgroup, but the loads go through a
    // pointer that is itself loaded, so the compiler makes them vector loads and every test on them a vector compare under
    // an exec mask; readfirstlane puts them where the kernel arguments were, in SGPRs (scalar compares and branches)
    const rsseg_forest_job *jp = a.jobs + t;
    const int max_depth = ff_uniform(jp->max_depth), mss = ff_uniform(jp->min_samples_split), msl = ff_uniform(jp->min_samples_leaf);
    const int max_features = ff_uniform(jp->max_features);
    const int weight_total = ff_uniform((int)jp->weight_total);   // below 2^26
    const int32_t *cnt = a.counts + (int64_t)ff_uniform((int)jp->counts_row) * a.n;   // the host keeps the row count below 2^31
    int32_t *smp = a.samples + a.samp_off[t];
    const int64_t so = a.samp_off[t];
    uint64_t *g0 = a.g0 + so, *g1 = a.g1 + so;
    const int64_t no = a.node_off[t], ncap = a.node_off[t + 1] - a.node_off[t];
    ff_entry *stk = a.stack + a.stack_off[t];
    const int64_t scap = a.stack_off[t + 1] - a.stack_off[t];
    const int F = a.F, C = a.C;
    const double w_total = (double)weight_total;   // weighted_n_samples: the bootstrap draws, or the unit weights, of the tree's training set
    if (tid < FF_MAX_F) {
        S.features[tid] = st->features[tid];
        S.constants[tid] = st->constants[tid];
    }
    if (tid == 0) {
        S.rng = st->rng;
        S.node_count = st->node_count;
        S.stack_size = st->stack_size;
        S.max_depth_seen = st->max_depth_seen;
        S.err = 0;
    }
    __syncthreads();
    for (int it = 0; it < a.budget; it++) {
        const bool stop = S.stack_size == 0 || S.err;
        __syncthreads();
        if (stop) break;
        if (tid == 0) {
            if (S.node_count >= ncap) S.err = 2;   // never with the host's 2m-1 sizing
            S.cur = stk[--S.stack_size];
        }
        if (tid < C) S.tot[tid] = 0;
        __syncthreads();
        if (S.err) break;
        const ff_entry cur = S.cur;
        const int n = cur.end - cur.start;
        const int32_t *ns = smp + cur.start;
        for (int i = tid; i < n; i += FF_THREADS) {
            const int s = ns[i];
            atomicAdd(&S.tot[a.y[s]], cnt[s]);
        }
        __syncthreads();
        if (tid == 0) {
            long long wsum = 0, sq = 0;
            for (int c = 0; c < C; c++) {
                wsum += S.tot[c];
                sq += (long long)S.tot[c] * S.tot[c];
            }
            S.wsum = (int)wsum;
            S.sq = sq;
            if (cur.impurity < 0.0) {   // the root: node_impurity
                const double wd = (double)wsum;
                S.cur.impurity = 1.0 - (double)sq / (wd * wd);
            }
        }
        __syncthreads();
        const double impurity = S.cur.impurity;
        const long long W = S.wsum;
        bool leaf = cur.depth >= max_depth || n < mss || n < 2 * msl || impurity <= DBL_EPSILON;
        if (tid == 0) {
            S.best.score = -INFINITY;
            S.best.pos = n;   // "no split": pos >= end
            S.best_feature = -1;
            S.f_i = F;
            S.nvis = 0;
            S.nfound = 0;
            S.ndrawn = 0;
            S.nknown = cur.n_const;
            S.ntotal = cur.n_const;
        }
        __syncthreads();
        if (!leaf) {
            // node_split_best's draw loop; thread 0 owns the draw state, the workgroup evaluates each drawn feature
            for (int guard = 0; guard < 2 * FF_MAX_F + 2; guard++) {
                if (tid == 0) {
                    if (S.f_i > S.ntotal && (S.nvis < max_features || S.nvis <= S.nfound + S.ndrawn)) {
                        S.nvis++;
                        int fj = ff_rand_int(S.ndrawn, S.f_i - S.nfound, &S.rng);
                        if (fj < S.nknown) {
                            const int x = S.features[S.ndrawn];
                            S.features[S.ndrawn] = S.features[fj];
                            S.features[fj] = x;
                            S.ndrawn++;
                            S.action = FF_SKIP;
                        } else {
                            fj += S.nfound;
                            S.fj = fj;
                            S.fcur = S.features[fj];
                            S.action = FF_EVAL;
                        }
                    } else {
                        S.action = FF_STOP;
                    }
                }
                __syncthreads();
                const int action = S.action;
                if (action == FF_STOP) break;
                if (action == FF_EVAL) {
                    const int f = S.fcur;
                    const uint64_t *buf = ff_sort(a, S, ns, n, a.planes[f], g0, g1);
                    const float lo = ff_val(buf[0]), hi = ff_val(buf[n - 1]);
                    const bool is_const = ff_close(lo, hi);
                    ff_best b;
                    if (!is_const) b = ff_scan(a, S, buf, n, cnt, W, msl);
                    if (tid == 0) {
                        if (is_const) {
                            const int x = S.features[S.fj];
                            S.features[S.fj] = S.features[S.ntotal];
                            S.features[S.ntotal] = x;
                            S.nfound++;
                            S.ntotal++;
                        } else {
                            S.f_i--;
                            const int x = S.features[S.f_i];
                            S.features[S.f_i] = S.features[S.fj];
                            S.features[S.fj] = x;
                            if (b.pos < n && b.score > S.best.score) {
                                S.best = b;
                                S.best_feature = f;
                                S.b_lo = ff_val(buf[b.pos - 1]);
                                S.b_hi = ff_val(buf[b.pos]);
                            }
                        }
                    }
                }
                __syncthreads();
            }
            if (tid == 0) {
                // memcpy of the known constants back, newly found constants appended (_splitter.pyx:537-543)
                for (int i = 0; i < S.nknown; i++) S.features[i] = S.constants[i];
                for (int i = 0; i < S.nfound; i++) S.constants[S.nknown + i] = S.features[S.nknown + i];
            }
            __syncthreads();
        }
        // split or leaf
        const bool found = !leaf && S.best_feature >= 0;
        double thr = 0.0;
        bool is_split = false;
        if (found) {
            const ff_best b = S.best;
            const double wn = (double)W, wl = (double)b.wl, wr = (double)(W - b.wl);
            const double improvement = (wn / w_total) * (impurity - (wr / wn * b.gr) - (wl / wn * b.gl));
            is_split = !(improvement + DBL_EPSILON < 0.0);
            thr = (double)S.b_lo / 2.0 + (double)S.b_hi / 2.0;
            if (thr == (double)S.b_hi || thr == INFINITY || thr == -INFINITY) thr = (double)S.b_lo;
        }
        if (is_split) {
            // partition_samples_final: X[s, f] <= threshold to the left; ordered compaction through g0
            const float *plane = a.planes[S.best_feature];
            int32_t *tmp = (int32_t *)g0;
            int nl_seen = 0;
            for (int c0 = 0; c0 < n; c0 += FF_THREADS) {
                const int i = c0 + tid;
                int s = 0, gl = 0;
                if (i < n) {
                    s = ns[i];
                    gl = ((double)plane[s] <= thr) ? 1 : 0;
                }
                int tot;
                const int off = block_excl_count(gl, S.s_w, &tot);
                if (i < n) {
                    const int o = gl ? nl_seen + off : S.best.pos + (c0 - nl_seen) + (tid - off);
                    if (o >= 0 && o < n) tmp[o] = s;
                }
                nl_seen += tot;
            }
            __threadfence_block();
            __syncthreads();
            for (int i = tid; i < n; i += FF_THREADS) smp[cur.start + i] = tmp[i];
            if (tid == 0 && nl_seen != S.best.pos) S.err = 3;
            __threadfence_block();
            __syncthreads();
        }
        // record the node (Tree._add_node) and push the children (right first, then left)
        if (tid == 0) {
            const int64_t id = S.node_count++;
            const int64_t g = no + id;
            if (cur.parent >= 0) {
                if (cur.is_left) a.left[no + cur.parent] = (int32_t)id;
                else a.right[no + cur.parent] = (int32_t)id;
            }
            a.left[g] = -1;
            a.right[g] = -1;
            a.impurity[g] = impurity;
            a.n_node[g] = n;
            a.w_node[g] = (int32_t)W;
            if (is_split) {
                a.feature[g] = S.best_feature;
                a.threshold[g] = thr;
                a.missing_left[g] = S.best.pos > n - S.best.pos ? 1 : 0;
                if (S.stack_size + 2 > scap) {
                    S.err = 4;
                } else {
                    const int nc = S.ntotal;
                    ff_entry r = {cur.start + S.best.pos, cur.end, cur.depth + 1, (int)id, 0, nc, S.best.gr};
                    ff_entry l = {cur.start, cur.start + S.best.pos, cur.depth + 1, (int)id, 1, nc, S.best.gl};
                    stk[S.stack_size++] = r;
                    stk[S.stack_size++] = l;
                }
            } else {
                a.feature[g] = -2;
                a.threshold[g] = -2.0;
                a.missing_left[g] = 0;
            }
            if (cur.depth > S.max_depth_seen) S.max_depth_seen = cur.depth;
        }
        __syncthreads();
        if (tid < C) a.value[(no + S.node_count - 1) * C + tid] = (double)S.tot[tid] / (double)W;
        __syncthreads();
    }
    if (tid < FF_MAX_F) {
        st->features[tid] = S.features[tid];
        st->constants[tid] = S.constants[tid];
    }
    if (tid == 0) {
        st->rng = S.rng;
        st->node_count = S.node_count;
        st->stack_size = S.stack_size;
        st->max_depth_seen = S.max_depth_seen;
        st->err = S.err;
        st->done = (S.stack_size == 0 || S.err) ? 1 : 0;
    }
}

}  // namespace

static int ff_check_shape(rsseg_ctx *ctx, const char *who, int F, int n_classes)
{
    if (F < 1 || F > FF_MAX_F || n_classes < 1 || n_classes > FF_MAX_C)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "%s: %d features, %d classes: at most %d of each", who, F, n_classes, FF_MAX_F);
    return RSSEG_OK;
}

// The body of both entry points: `who` names the caller in messages and in the profiler; `uniform` is rsseg_forest_fit, whose
// jobs all have weight_total = n (it keeps its own wording for a count row with another sum).
static int ff_run(rsseg_ctx *ctx, const char *who, bool uniform, const float *const *d_planes, int F, int64_t n, const int32_t *d_y,
                  int n_classes, const int32_t *d_counts, int64_t n_count_rows, int n_trees, const rsseg_forest_job *jobs,
                  const int64_t *node_off, int32_t *d_left, int32_t *d_right, int32_t *d_feature, double *d_threshold,
                  double *d_impurity, int32_t *d_n_node, int32_t *d_w_node, uint8_t *d_missing_left, double *d_value,
                  int64_t *node_count, int32_t *max_depth_out)
{
    RSCHK(ff_check_shape(ctx, who, F, n_classes));
    if (n < 1 || n >= (int64_t)1 << 26 || n_trees < 1 || n_count_rows < 1 || n_count_rows > INT32_MAX || !d_planes || !d_y || !d_counts || !jobs || !node_off ||
        !node_count || !max_depth_out)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: bad arguments (n=%lld trees=%d count rows=%lld; 1 <= n < 2^26)", who, (long long)n,
                       n_trees, (long long)n_count_rows);
    ff_args a;
    memset(&a, 0, sizeof(a));
    for (int f = 0; f < F; f++)
        if (!d_planes[f]) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: plane %d is NULL", who, f);
    // per-tree sample counts m_t (the host passes node_off = prefix of 2 m_t - 1): the layout follows from it
    std::vector<int64_t> samp(n_trees + 1, 0), stk(n_trees + 1, 0);
    for (int t = 0; t < n_trees; t++) {
        const rsseg_forest_job &j = jobs[t];
        if (j.counts_row < 0 || j.counts_row >= n_count_rows || j.weight_total < 1 || j.weight_total >= (int64_t)1 << 26 || j.max_depth < 0 ||
            j.min_samples_split < 2 || j.min_samples_leaf < 1 || j.max_features < 0)
            return rs_fail(ctx, RSSEG_ERR_INVALID,
                           "%s: tree %d: bad job (counts_row=%lld of %lld rows, weight_total=%lld, max_depth=%d min_samples_split=%d "
                           "min_samples_leaf=%d max_features=%d; 1 <= weight_total < 2^26)", who, t, (long long)j.counts_row,
                           (long long)n_count_rows, (long long)j.weight_total, j.max_depth, j.min_samples_split, j.min_samples_leaf,
                           j.max_features);
        const int64_t cap = node_off[t + 1] - node_off[t];
        if (cap < 1 || !(cap & 1)) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: tree %d: node capacity %lld is not 2m-1", who, t, (long long)cap);
        const int64_t m = (cap + 1) / 2;
        if (m > n) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: tree %d: %lld samples > n", who, t, (long long)m);
        samp[t + 1] = samp[t] + m;
        stk[t + 1] = stk[t] + std::min<int64_t>(j.max_depth, m) + 2;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t b_off = 3 * 8 * (size_t)(n_trees + 1), b_job = sizeof(rsseg_forest_job) * (size_t)n_trees, b_pl = 8 * (size_t)F, b_args = sizeof(ff_args);
    const size_t b_smp = 4 * (size_t)samp[n_trees], b_g = 8 * (size_t)samp[n_trees];
    const size_t b_st = sizeof(ff_state) * n_trees, b_stk = sizeof(ff_entry) * (size_t)stk[n_trees];
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t total = al(b_args) + al(b_off) + al(b_job) + al(b_pl) + al(b_smp) + 2 * al(b_g) + al(b_st) + al(b_stk);
    RSCHK(ws_reserve(ctx, total));
    char *p = ctx->d_ws;
    ff_args *d_args = (ff_args *)p; p += al(b_args);
    int64_t *d_off = (int64_t *)p; p += al(b_off);
    rsseg_forest_job *d_job = (rsseg_forest_job *)p; p += al(b_job);
    const float **d_pl = (const float **)p; p += al(b_pl);
    a.samples = (int32_t *)p; p += al(b_smp);
    a.g0 = (uint64_t *)p; p += al(b_g);
    a.g1 = (uint64_t *)p; p += al(b_g);
    a.st = (ff_state *)p; p += al(b_st);
    a.stack = (ff_entry *)p;
    std::vector<int64_t> hoff(3 * (n_trees + 1));
    for (int t = 0; t <= n_trees; t++) {
        hoff[t] = samp[t];
        hoff[n_trees + 1 + t] = node_off[t];
        hoff[2 * (n_trees + 1) + t] = stk[t];
    }
    HIPCHK(ctx, hipMemcpyAsync(d_off, hoff.data(), b_off, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_job, jobs, b_job, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_pl, d_planes, b_pl, hipMemcpyHostToDevice, ctx->stream));
    a.planes = d_pl;
    a.samp_off = d_off;
    a.node_off = d_off + (n_trees + 1);
    a.stack_off = d_off + 2 * (n_trees + 1);
    a.jobs = d_job;
    a.y = d_y;
    a.counts = d_counts;
    a.n = n;
    a.F = F;
    a.C = n_classes;
    a.T = n_trees;
    a.budget = 2048;
    a.left = d_left;
    a.right = d_right;
    a.feature = d_feature;
    a.threshold = d_threshold;
    a.impurity = d_impurity;
    a.n_node = d_n_node;
    a.w_node = d_w_node;
    a.missing_left = d_missing_left;
    a.value = d_value;

    // the arguments live in device memory: the kernels read the fields they need instead of holding ~30 pointers in SGPRs
    HIPCHK(ctx, hipMemcpyAsync(d_args, &a, b_args, hipMemcpyHostToDevice, ctx->stream));
    prof_scope ps(ctx, who);
    hipLaunchKernelGGL(k16_fit_init, dim3(n_trees), dim3(FF_THREADS), 0, ctx->stream, (const ff_args *)d_args);
    HIPCHK(ctx, hipGetLastError());
    RSCHK(pin_reserve(ctx, b_st));
    ff_state *h = (ff_state *)ctx->h_pin;
    int64_t max_nodes = 0;
    for (int t = 0; t < n_trees; t++) max_nodes = std::max(max_nodes, node_off[t + 1] - node_off[t]);
    const int64_t max_launches = ceil_div64(max_nodes, a.budget) + 2;
    int64_t prev = -1;
    for (int64_t launch = 0;; launch++) {
        if (launch >= max_launches)
            return rs_fail(ctx, RSSEG_ERR_HIP, "%s: %lld launches did not finish the trees", who, (long long)launch);
        hipLaunchKernelGGL(k16_fit_step, dim3(n_trees), dim3(FF_THREADS), 0, ctx->stream, (const ff_args *)d_args);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(h, a.st, b_st, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, rs_sync(ctx));
        int64_t built = 0;
        bool all = true;
        for (int t = 0; t < n_trees; t++) {
            if (h[t].err == 5 && uniform)
                return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: tree %d: the counts are negative or do not sum to n = %lld "
                               "(weighted_n_samples is n)", who, t, (long long)n);
            if (h[t].err == 5)
                return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: tree %d: the counts of row %lld are negative or do not sum to weight_total = %lld "
                               "(the tree's weighted_n_samples)", who, t, (long long)jobs[t].counts_row, (long long)jobs[t].weight_total);
            if (h[t].err)
                return rs_fail(ctx, RSSEG_ERR_NOMEM, "%s: tree %d stopped with error %d after %d nodes (%s)", who, t, h[t].err, h[t].node_count,
                               h[t].err == 1 ? "sample count mismatch" : h[t].err == 2 ? "node storage full" : h[t].err == 3 ? "inconsistent partition" : "stack full");
            built += h[t].node_count;
            all = all && h[t].done;
        }
        if (all) break;
        if (built <= prev) return rs_fail(ctx, RSSEG_ERR_HIP, "%s: launch %lld made no progress", who, (long long)launch);
        prev = built;
    }
    for (int t = 0; t < n_trees; t++) {
        node_count[t] = h[t].node_count;
        max_depth_out[t] = h[t].max_depth_seen;
    }
    return RSSEG_OK;
}

extern "C" int rsseg_forest_fit_jobs(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_y, int n_classes,
                                     const int32_t *d_counts, int64_t n_count_rows, int n_trees, const rsseg_forest_job *jobs,
                                     const int64_t *node_off, int32_t *d_left, int32_t *d_right, int32_t *d_feature, double *d_threshold,
                                     double *d_impurity, int32_t *d_n_node, int32_t *d_w_node, uint8_t *d_missing_left, double *d_value,
                                     int64_t *node_count, int32_t *max_depth_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    return ff_run(ctx, "forest_fit_jobs", false, d_planes, F, n, d_y, n_classes, d_counts, n_count_rows, n_trees, jobs, node_off, d_left, d_right,
                  d_feature, d_threshold, d_impurity, d_n_node, d_w_node, d_missing_left, d_value, node_count, max_depth_out);
}

// the uniform case: one set of parameters, tree t on count row t (or all on row 0), weight_total = n
extern "C" int rsseg_forest_fit(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_y, int n_classes,
                                const int32_t *d_counts, int same_counts, int n_trees, const uint32_t *seeds, int max_depth,
                                int min_samples_split, int min_samples_leaf, int max_features, const int64_t *node_off,
                                int32_t *d_left, int32_t *d_right, int32_t *d_feature, double *d_threshold, double *d_impurity,
                                int32_t *d_n_node, int32_t *d_w_node, uint8_t *d_missing_left, double *d_value,
                                int64_t *node_count, int32_t *max_depth_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    RSCHK(ff_check_shape(ctx, "forest_fit", F, n_classes));
    if (n < 1 || n >= (int64_t)1 << 26 || n_trees < 1 || !d_planes || !d_y || !d_counts || !seeds || !node_off || !node_count ||
        !max_depth_out || max_depth < 0 || min_samples_split < 2 || min_samples_leaf < 1 || max_features < 0)
        return rs_fail(ctx, RSSEG_ERR_INVALID,
                       "forest_fit: bad arguments (n=%lld trees=%d max_depth=%d min_samples_split=%d min_samples_leaf=%d max_features=%d; "
                       "1 <= n < 2^26)", (long long)n, n_trees, max_depth, min_samples_split, min_samples_leaf, max_features);
    std::vector<rsseg_forest_job> jobs(n_trees);
    for (int t = 0; t < n_trees; t++) {
        rsseg_forest_job &j = jobs[t];
        j.counts_row = same_counts ? 0 : t;
        j.weight_total = n;
        j.seed = seeds[t];
        j.max_depth = max_depth;
        j.min_samples_split = min_samples_split;
        j.min_samples_leaf = min_samples_leaf;
        j.max_features = max_features;
        j.reserved = 0;
    }
    return ff_run(ctx, "forest_fit", true, d_planes, F, n, d_y, n_classes, d_counts, same_counts ? 1 : n_trees, n_trees, jobs.data(), node_off, d_left,
                  d_right, d_feature, d_threshold, d_impurity, d_n_node, d_w_node, d_missing_left, d_value, node_count, max_depth_out);
}
