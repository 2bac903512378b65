// K11, permutation importance: how many samples the loaded forest still labels correctly when one feature column is
// taken from another row.
//
// Replaces the F * n_repeats + 1 calls of RandomForestClassifier.predict inside sklearn.inspection.permutation_importance
// (inspection/_permutation_importance.py:43-85: a column shuffled cumulatively, the estimator scored after every shuffle;
// scoring = accuracy, whose numerator is the count below).  For job j = (feature f, source row s), f = -1: no substitution,
//   counts[j] = #{ i < n : label_index(x_i with x_i[f] := planes[f][src[s * n + i]]) == y[i] }
// label_index: what rsseg_forest_predict turns into classes[...] (float64 sums of the leaf rows in tree order, divided by
// the tree count, first maximum on ties); y[i] = -1 (a label the forest does not know) is never correct.
//
// The node layout, the vote table, the walks and the launch path are those of k11_forest.h; the two kernels below are
// k11_forest_lds and k11_forest_gen with another staging and another finish, written out (DESIGN.md section 5 says why they
// are not one body).  Jobs sit on blockIdx.y: a workgroup is (a block of RF_TH samples, one job).
//   staging   the sample's own features, except feature f, which comes from row src[s * n + i] of the same plane.  The
//             NaN-aware walk is chosen from the values staged, AFTER the substitution: a NaN brought in from a row of
//             another workgroup turns it on, a NaN that the substitution replaced does not.  A source index outside
//             [0, n) is not dereferenced: the lane stages 0 and raises *flag.
//   finish    argmax == y[i] per lane, summed in integers over the wave and the workgroup, then one 64-bit atomic add per
//             workgroup into counts[j]: integer addition in any order gives the same count.
// Why blockIdx.y and not a loop over jobs inside the workgroup: staging is 4F B of the ~100-tree walk's work per sample
// (the walk is VALU-issue-bound, k11_forest.hip), so sharing it between jobs saves nothing measurable, while the vote
// accumulators of several jobs (NC doubles each) would not fit the registers beside the RF_C chains; and at the sizes
// the call is made for (m samples of an ROI, F * n_repeats + 1 ~ 100 jobs) it is the jobs that fill the 256 CUs.
// HBM traffic per job: 4F B/sample in (the planes; L2-resident across jobs at ROI sizes) + 4 B (y) + 4 B (src) + 4 B (the
// substituted value, a gather), 8 B per workgroup out.
#include "common.h"
#include "k11_forest.h"

struct rf_perm_args {
    const int32_t *y;                 // [n] class index, -1: unknown label
    const int32_t *src;               // [n_src][n] source rows
    const rsseg_perm_job *jobs;       // device copy; blockIdx.y indexes it
    unsigned long long *counts;       // one per job, zero before the launch
    int *flag;                        // raised when a source index is outside [0, n)
};

// the value the job puts in place of feature `fj` of sample i (0 where there is nothing to read)
__device__ __forceinline__ float rf_perm_value(const rf_planes &pl, const rf_perm_args &a, const rsseg_perm_job job, int64_t n, int64_t i)
{
    float v = 0.f;
    if (job.feature >= 0 && i < n) {
        const int32_t s = a.src[(size_t)job.source * (size_t)n + (size_t)i];
        if (s < 0 || (int64_t)s >= n) *a.flag = 1;
        else v = pl.p[job.feature][s];
    }
    return v;
}

template <int NC, int RF_TH>
__device__ __forceinline__ void rf_perm_finish(const double (&acc)[NC], int n_trees, int n_classes, const rf_perm_args &a, int64_t n, int64_t i,
                                               int *s_ok /* LDS, RF_TH / WAVE ints, free once every wave has passed the barrier below */)
{
    int ok = 0;
    if (i < n) {
        int best = 0;
        double bv = acc[0] / (double)n_trees;
#pragma unroll
        for (int c = 1; c < NC; c++)
            if (c < n_classes) {
                const double p = acc[c] / (double)n_trees;
                if (p > bv) { bv = p; best = c; }
            }
        ok = best == a.y[i] ? 1 : 0;
    }
    // the partial sums go where the features were (the dynamic LDS is sized to the byte: no static array beside it)
    __syncthreads();   // every wave is done walking
    ok = wave_sum(ok);
    if (lane_id() == 0) s_ok[threadIdx.x >> 6] = ok;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RF_TH / WAVE; w++) ok += s_ok[w];
        if (ok) atomicAdd(&a.counts[blockIdx.y], (unsigned long long)ok);
    }
}

// k11_forest_perm_lds keeps its LDS-group body WRITTEN OUT, as the parent had it: as a policy on a shared __forceinline__ body it computed
// the same values, but was over the speed bar in two of three sessions.  The three LDS-group kernels (here, k11_forest_proba.hip,
// k11_forest_perm.hip) share the walks, the vote rows, RF_PRE / RF_PUT and the launch path of k11_forest.h; a change to the
// steps of one body is made in the other two as well.
template <int NC, int RF_TH>
__global__ __launch_bounds__(RF_TH) void k11_forest_perm_lds(rf_planes pl, int F, int64_t n, const rf_node *__restrict__ nodes,
                                                             const rf_tree *__restrict__ trees, const rf_group *__restrict__ groups, int n_groups,
                                                             int cap2 /* node area in 16-byte pieces */, int two_rounds, int n_trees,
                                                             const double *__restrict__ leafval, int n_classes, rf_perm_args a)
{
    extern __shared__ __align__(16) char smem[];
    const int FP = F | 1;
    float *feat = reinterpret_cast<float *>(smem);                             // [RF_TH samples][FP]
    uint4 *top = reinterpret_cast<uint4 *>(feat + (size_t)FP * RF_TH);         // the current group's nodes, two per uint4
    const int64_t i0 = (int64_t)blockIdx.x * RF_TH + threadIdx.x;
    const rsseg_perm_job job = a.jobs[blockIdx.y];
    const float sub = rf_perm_value(pl, a, job, n, i0);
    int my_nan = 0;
    for (int f = 0; f < F; f++) {
        const float v = f == job.feature ? sub : (i0 < n ? pl.p[f][i0] : 0.f);
        my_nan |= v != v;
        feat[threadIdx.x * FP + f] = v;
    }
    {
        const rf_group g0 = groups[0];
        const uint4 *src = reinterpret_cast<const uint4 *>(nodes + g0.node_base);
        for (int j = threadIdx.x; j < (g0.n_nodes + 1) / 2; j += RF_TH) top[j] = src[j];
        if (threadIdx.x == 0) top[cap2] = make_uint4(RF_NAN_BITS, RF_LEAF | RF_MISS, RF_NAN_BITS, RF_LEAF | RF_MISS);
    }
    const bool any_nan = __syncthreads_or(my_nan) != 0;   // of the values staged for THIS job
    const unsigned feat_tid = (unsigned)(uintptr_t)(lds_cfloat *)feat + threadIdx.x * (unsigned)FP * 4u;
    const unsigned top_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const uint4 *)top;
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0;
    for (int g = 0; g < n_groups; g++) {
        const rf_group gr = groups[g];
        // the next group's nodes in the six named registers of k11_forest.h (RF_PRE / RF_PUT)
        static_assert(RF_NPRE == 6, "the prefetch registers below are spelled out for six pieces per thread");
        const bool more = g + 1 < n_groups;
        const rf_group gn = groups[more ? g + 1 : g];
        const int npiece = more ? (gn.n_nodes + 1) / 2 : 0;
        const uint4 *psrc = reinterpret_cast<const uint4 *>(nodes + gn.node_base);
        const int plast = (gn.n_nodes + 1) / 2 - 1;
        RF_PRE(0) RF_PRE(1) RF_PRE(2) RF_PRE(3) RF_PRE(4) RF_PRE(5)
        rf_node nd[RF_C];
        unsigned base[RF_C];
#pragma unroll
        for (int c = 0; c < RF_C; c++) {
            const rf_tree tr = trees[c < gr.count ? gr.first + c : gr.first];
            base[c] = c < gr.count ? top_addr + (unsigned)(tr.node_off - gr.node_base) * 8u : top_addr + (unsigned)cap2 * 16u;
            lds_cnode *p = RF_LDS_PTR(lds_cnode, base[c]);
            nd[c].thr = p->thr;
            nd[c].bits = p->bits;
        }
        if (any_nan) rf_walk_lds<true>(nd, feat_tid, base, two_rounds != 0);
        else rf_walk_lds<false>(nd, feat_tid, base, two_rounds != 0);
        // refill first, then the vote rows of all chains at once, added in tree order behind the barrier (k11_forest_lds)
        constexpr bool PIPE = NC <= 8;
        double rows[PIPE ? RF_C : 1][NC];
        if (PIPE) {
#pragma unroll
            for (int q = 0; q < RF_C; q++) rf_row_load<NC>(nd[q], leafval, rows[PIPE ? q : 0]);
        } else {
#pragma unroll
            for (int q = 0; q < RF_C; q++)
                if (q < gr.count && i0 < n) rf_vote_pieces<NC>(nd[q], leafval, acc);
        }
        if (more) {
            __syncthreads();  // every wave is done with the current group
            RF_PUT(0) RF_PUT(1) RF_PUT(2) RF_PUT(3) RF_PUT(4) RF_PUT(5)
        }
        if (more) __syncthreads();
        if (PIPE) {
#pragma unroll
            for (int q = 0; q < RF_C; q++)
                if (q < gr.count) {   // lanes without a sample add the rows of their zero features and count nothing
#pragma unroll
                    for (int c = 0; c < NC; c++) acc[c] += rows[PIPE ? q : 0][c];
                }
        }
    }
    rf_perm_finish<NC, RF_TH>(acc, n_trees, n_classes, a, n, i0, reinterpret_cast<int *>(smem));
}

// the general kernel, written out like the LDS-group one above (as a policy on a shared body it did not keep the parent's
// speed: DESIGN.md section 5); a change to its steps is made in the other two files as well
template <int NC, int RF_TH>
__global__ __launch_bounds__(RF_TH) void k11_forest_perm_gen(rf_planes pl, int F, int64_t n, const rf_node *__restrict__ nodes,
                                                             const rf_tree *__restrict__ trees, int n_trees, int ntop,
                                                             const double *__restrict__ leafval, int n_classes, rf_perm_args a)
{
    extern __shared__ __align__(16) char smem[];
    float *feat = reinterpret_cast<float *>(smem);                                   // [F][RF_TH]
    rf_node *top = reinterpret_cast<rf_node *>(feat + (size_t)F * RF_TH);            // [RF_C][ntop]
    const int64_t i = (int64_t)blockIdx.x * RF_TH + threadIdx.x;
    const rsseg_perm_job job = a.jobs[blockIdx.y];
    const float sub = rf_perm_value(pl, a, job, n, i);
    int my_nan = 0;
    for (int f = 0; f < F; f++) {
        const float v = f == job.feature ? sub : (i < n ? pl.p[f][i] : 0.f);
        my_nan |= v != v;
        feat[f * RF_TH + threadIdx.x] = v;
    }
    constexpr int NPRE = 12;  // RF_C * ntop <= 12 * RF_TH nodes per group (the host keeps ntop <= 3 * RF_TH)
    // 32 accumulators at 1024 threads are 64 of a lane's 128 registers: the next group's nodes (24 more) do not fit beside the
    // walk without scratch memory, so that one width fetches them behind the barrier instead of holding them across the walk
    constexpr bool PRE = !(NC >= 32 && RF_TH == 1024);
    for (int c = 0; c < RF_C && c < n_trees; c++) {
        const rf_tree t0 = trees[c];
        const int cnt = t0.n_nodes < ntop ? t0.n_nodes : ntop;
        for (int j = threadIdx.x; j < cnt; j += RF_TH) top[(size_t)c * ntop + j] = nodes[t0.node_off + j];
    }
    const bool any_nan = __syncthreads_or(my_nan) != 0;   // of the values staged for THIS job
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0;
    const int n_groups = (n_trees + RF_C - 1) / RF_C;
    for (int g = 0; g < n_groups; g++) {
        const int t = g * RF_C;
        rf_tree tr[RF_C];
#pragma unroll
        for (int c = 0; c < RF_C; c++) tr[c] = trees[t + c < n_trees ? t + c : n_trees - 1];
        rf_node pre[NPRE];
        int pcnt[RF_C], poff[RF_C];
        const bool more = t + RF_C < n_trees;
        if (more) {
#pragma unroll
            for (int c = 0; c < RF_C; c++) {
                const bool have = t + RF_C + c < n_trees;
                const rf_tree tnx = trees[have ? t + RF_C + c : n_trees - 1];
                pcnt[c] = have ? (tnx.n_nodes < ntop ? tnx.n_nodes : ntop) : 0;
                poff[c] = tnx.node_off;
            }
#pragma unroll
            for (int r = 0; PRE && r < NPRE; r++) {
                const int j = threadIdx.x + r * RF_TH;  // [0, RF_C * ntop): block c = j / ntop
                if (j < RF_C * ntop) {
                    const int c = j / ntop, o2 = j - c * ntop;
                    int cnt = pcnt[0], off = poff[0];
#pragma unroll
                    for (int cc = 1; cc < RF_C; cc++)
                        if (c == cc) { cnt = pcnt[cc]; off = poff[cc]; }
                    if (o2 < cnt) pre[r] = nodes[off + o2];
                }
            }
        }
        {
            rf_node nd[RF_C];
            int lim[RF_C], noff[RF_C];
            lds_cfloat *lfeat = (lds_cfloat *)feat;
            lds_cnode *ltop = (lds_cnode *)top;
#pragma unroll
            for (int c = 0; c < RF_C; c++) {
                noff[c] = tr[c].node_off;
                lim[c] = tr[c].n_nodes < ntop ? tr[c].n_nodes : ntop;
                nd[c].thr = ltop[c * ntop].thr;
                nd[c].bits = ltop[c * ntop].bits;
                if (t + c >= n_trees || i >= n) nd[c].bits = RF_LEAF;  // no tree / no sample: nothing to walk
            }
            if (any_nan) rf_walk_gen<true, RF_TH>(nd, lfeat, ltop, ntop, lim, nodes, noff);
            else rf_walk_gen<false, RF_TH>(nd, lfeat, ltop, ntop, lim, nodes, noff);
            if (i < n) {
#pragma unroll
                for (int c = 0; c < RF_C; c++)
                    if (t + c < n_trees) rf_vote_pieces<NC>(nd[c], leafval, acc);
            }
        }
        if (more) {
            __syncthreads();  // every wave is done with the current blocks
#pragma unroll
            for (int r = 0; r < NPRE; r++) {
                const int j = threadIdx.x + r * RF_TH;
                if (j < RF_C * ntop) {
                    const int c = j / ntop, o2 = j - c * ntop;
                    int cnt = pcnt[0], off = poff[0];
#pragma unroll
                    for (int cc = 1; cc < RF_C; cc++)
                        if (c == cc) { cnt = pcnt[cc]; off = poff[cc]; }
                    if (o2 < cnt) {
                        if constexpr (PRE) top[j] = pre[r];
                        else top[j] = nodes[off + o2];
                    }
                }
            }
            __syncthreads();
        }
    }
    rf_perm_finish<NC, RF_TH>(acc, n_trees, n_classes, a, n, i, reinterpret_cast<int *>(smem));
}

// jobs [j0, j0 + nj) of the call in one launch: grid (blocks of TH samples, jobs), by the plan and the dispatch of k11_forest.h
static int rf_launch_perm(rsseg_ctx *ctx, const rf_planes &pl, int F, int64_t n, rf_perm_args a, int j0, int nj)
{
    const rf_plan p = rf_launch_plan(ctx->forest, F);
    a.jobs += j0;
    a.counts += j0;
    auto launch = [&](auto kern) { return rf_launch(ctx, p, "forest_perm", (unsigned)nj, kern, pl, F, n, a); };
    int rc = RSSEG_ERR_INVALID;
    if (p.lds_groups) { RF_DISPATCH(rc, p, launch, k11_forest_perm_lds) }
    else { RF_DISPATCH(rc, p, launch, k11_forest_perm_gen) }
    if (rc != RSSEG_OK) return rc;
    HIPCHK(ctx, hipGetLastError());
    return RSSEG_OK;
}

#define RF_PERM_MAX_GRID_Y 65535   // jobs per launch

extern "C" int rsseg_forest_permutation_counts(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_y,
                                               const int32_t *d_src, int n_src, const rsseg_perm_job *jobs, int n_jobs, int64_t *counts)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    const char *who = "forest_permutation_counts";
    rf_planes pl;
    RSCHK(rf_check_planes(ctx, who, d_planes, n >= 0 && n_jobs >= 0 && n_src >= 0, F, pl));
    if (!d_y) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: the labels are null", who);
    if (!jobs) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: the jobs are null", who);
    if (!counts) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: the counts are null", who);
    if (n >= (1LL << 31)) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: %lld samples exceed 2^31 - 1 (source rows are int32)", who, (long long)n);
    for (int j = 0; j < n_jobs; j++) {
        if (jobs[j].feature < -1 || jobs[j].feature >= F)
            return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: job %d has feature %d outside [-1, %d)", who, j, jobs[j].feature, F);
        if (jobs[j].feature < 0) continue;
        if (!d_src) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: the source rows are null, but job %d substitutes feature %d", who, j, jobs[j].feature);
        if (jobs[j].source < 0 || jobs[j].source >= n_src)
            return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: job %d has source %d outside [0, %d)", who, j, jobs[j].source, n_src);
    }
    if (n_jobs == 0) return RSSEG_OK;
    if (n == 0) {
        for (int j = 0; j < n_jobs; j++) counts[j] = 0;
        return RSSEG_OK;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // workspace: counts[n_jobs] and the flag (one 8-byte slot), zeroed on the stream, then the jobs; pinned: the same
    const size_t res_bytes = ((size_t)n_jobs + 1) * 8, job_bytes = (size_t)n_jobs * sizeof(rsseg_perm_job);
    RSCHK(ws_reserve(ctx, res_bytes + job_bytes));
    RSCHK(pin_reserve(ctx, res_bytes + job_bytes));
    rf_perm_args a;
    a.y = d_y;
    a.src = d_src;
    a.counts = (unsigned long long *)ctx->d_ws;
    a.flag = (int *)(a.counts + n_jobs);
    a.jobs = (const rsseg_perm_job *)(ctx->d_ws + res_bytes);
    long long *h_res = (long long *)ctx->h_pin;
    memcpy(ctx->h_pin + res_bytes, jobs, job_bytes);
    HIPCHK(ctx, hipMemsetAsync(ctx->d_ws, 0, res_bytes, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_ws + res_bytes, ctx->h_pin + res_bytes, job_bytes, hipMemcpyHostToDevice, ctx->stream));
    for (int j0 = 0; j0 < n_jobs; j0 += RF_PERM_MAX_GRID_Y)
        RSCHK(rf_launch_perm(ctx, pl, F, n, a, j0, std::min(n_jobs - j0, RF_PERM_MAX_GRID_Y)));
    HIPCHK(ctx, hipMemcpyAsync(h_res, ctx->d_ws, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    if (h_res[n_jobs] != 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: source index out of range [0, %lld)", who, (long long)n);
    for (int j = 0; j < n_jobs; j++) counts[j] = h_res[j];
    return RSSEG_OK;
}
