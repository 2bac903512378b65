// K11, the outputs beyond the label: class probabilities, confidence and the out-of-bag sums of the loaded forest.
//
// Replaces RandomForestClassifier.predict_proba (sklearn/ensemble/_forest.py:908-946: the trees' leaf rows added in tree
// order in float64, divided by the tree count) and ForestClassifier._compute_oob_predictions (_forest.py:558-622: the
// same sum over the trees whose bootstrap never drew the sample, divided by max(number of such trees, 1)).
//
// The node layout, the vote table, the walks and the launch path are those of k11_forest.h; the two kernels below are
// k11_forest_lds and k11_forest_gen with another finish, written out (DESIGN.md section 5 says why they are not one body):
//   OOB = false   proba[c][i] = acc[c] / n_trees (class-planar: for a class the lanes of a wave store consecutive
//                 doubles), conf[i] = the largest of them, labels[i] = classes[first maximum]; any output may be null
//   OOB = true    a tree's row is added, and the sample's count incremented, only where counts[tree][i] == 0; every chain
//                 is still walked (leaves are fixed points, nothing in the walk is conditional);
//                 oob[c][i] = acc[c] / max(n_oob, 1), n_oob[i] = the count.  A thread reads its sample's counts for the
//                 trees of a group before the walk: consecutive lanes, consecutive int32.
// HBM traffic: 4F B/px in, 8 * n_classes + 8 + 8 B/px out (proba, confidence, label); OOB adds 4 * n_trees B/sample in.
#include "common.h"
#include "k11_forest.h"

struct rf_outputs {
    double *proba;         // [n_classes][n]; the out-of-bag decision function when OOB
    double *conf;          // [n]
    long long *labels;     // [n]
    const int *counts;     // OOB: [n_trees][n] bootstrap counts
    int *n_oob;            // OOB: [n]
};

template <int NC, bool OOB>
__device__ __forceinline__ void rf_finish_out(const double (&acc)[NC], int n_trees, int n_oob, int n_classes,
                                              const long long *__restrict__ classes, const rf_outputs &o, int64_t n, int64_t i)
{
    const double den = OOB ? (double)(n_oob > 1 ? n_oob : 1) : (double)n_trees;
    int best = 0;
    double bv = acc[0] / den;
    if (o.proba) o.proba[i] = bv;
#pragma unroll
    for (int c = 1; c < NC; c++)
        if (c < n_classes) {
            const double p = acc[c] / den;
            if (o.proba) o.proba[(size_t)c * (size_t)n + (size_t)i] = p;
            if (p > bv) { bv = p; best = c; }
        }
    if (OOB) {
        o.n_oob[i] = n_oob;
    } else {
        if (o.conf) o.conf[i] = bv;
        if (o.labels) o.labels[i] = classes[best];
    }
}

// k11_forest_out_lds keeps its LDS-group body WRITTEN OUT, as the parent had it: as a policy on a shared __forceinline__ body it computed
// the same values, but missed the speed bar in two sessions.  The three LDS-group kernels (here, k11_forest_proba.hip,
// k11_forest_perm.hip) share the walks, the vote rows, RF_PRE / RF_PUT and the launch path of k11_forest.h; a change to the
// steps of one body is made in the other two as well.
template <int NC, int RF_TH, bool OOB>
__global__ __launch_bounds__(RF_TH) void k11_forest_out_lds(rf_planes pl, int F, int64_t n, const rf_node *__restrict__ nodes,
                                                            const rf_tree *__restrict__ trees, const rf_group *__restrict__ groups, int n_groups,
                                                            int cap2 /* node area in 16-byte pieces */, int two_rounds, int n_trees,
                                                            const double *__restrict__ leafval,
                                                            int n_classes, const long long *__restrict__ classes, rf_outputs o)
{
    extern __shared__ __align__(16) char smem[];
    const int FP = F | 1;
    float *feat = reinterpret_cast<float *>(smem);                             // [RF_TH pixels][FP]
    uint4 *top = reinterpret_cast<uint4 *>(feat + (size_t)FP * RF_TH);         // the current group's nodes, two per uint4
    const int64_t i0 = (int64_t)blockIdx.x * RF_TH + threadIdx.x;
    int my_nan = 0;
    for (int f = 0; f < F; f++) {
        const float v = i0 < n ? pl.p[f][i0] : 0.f;
        my_nan |= v != v;
        feat[threadIdx.x * FP + f] = v;
    }
    {
        const rf_group g0 = groups[0];
        const uint4 *src = reinterpret_cast<const uint4 *>(nodes + g0.node_base);
        for (int j = threadIdx.x; j < (g0.n_nodes + 1) / 2; j += RF_TH) top[j] = src[j];
        if (threadIdx.x == 0) top[cap2] = make_uint4(RF_NAN_BITS, RF_LEAF | RF_MISS, RF_NAN_BITS, RF_LEAF | RF_MISS);
    }
    const bool any_nan = __syncthreads_or(my_nan) != 0;
    const unsigned feat_tid = (unsigned)(uintptr_t)(lds_cfloat *)feat + threadIdx.x * (unsigned)FP * 4u;
    const unsigned top_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const uint4 *)top;
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0;
    int n_oob = 0;
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
        // out-of-bag: the sample's bootstrap counts for the trees of the group (a row of counts per tree: coalesced)
        bool use[RF_C];
#pragma unroll
        for (int c = 0; c < RF_C; c++) {
            use[c] = c < gr.count && i0 < n;
            if (OOB) {
                const int cnt = use[c] ? o.counts[(size_t)(gr.first + c) * (size_t)n + (size_t)i0] : 1;
                use[c] = cnt == 0;
                n_oob += use[c] ? 1 : 0;
            }
        }
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
                if (use[q]) rf_vote<NC>(nd[q], leafval, acc);
        }
        if (more) {
            __syncthreads();  // every wave is done with the current group
            RF_PUT(0) RF_PUT(1) RF_PUT(2) RF_PUT(3) RF_PUT(4) RF_PUT(5)
        }
        if (more) __syncthreads();
        if (PIPE) {
#pragma unroll
            for (int q = 0; q < RF_C; q++)
                if (OOB ? use[q] : q < gr.count) {   // lanes without a pixel add the rows of their zero features and store nothing
#pragma unroll
                    for (int c = 0; c < NC; c++) acc[c] += rows[PIPE ? q : 0][c];
                }
        }
    }
    if (i0 < n) rf_finish_out<NC, OOB>(acc, n_trees, n_oob, n_classes, classes, o, n, i0);
}

// the general kernel, written out like the LDS-group one above (as a policy on a shared body it did not keep the parent's
// speed: DESIGN.md section 5); a change to its steps is made in the other two files as well
template <int NC, int RF_TH, bool OOB>
__global__ __launch_bounds__(RF_TH) void k11_forest_out_gen(rf_planes pl, int F, int64_t n, const rf_node *__restrict__ nodes,
                                                            const rf_tree *__restrict__ trees, int n_trees, int ntop,
                                                            const double *__restrict__ leafval, int n_classes,
                                                            const long long *__restrict__ classes, rf_outputs o)
{
    extern __shared__ __align__(16) char smem[];
    float *feat = reinterpret_cast<float *>(smem);                                   // [F][RF_TH]
    rf_node *top = reinterpret_cast<rf_node *>(feat + (size_t)F * RF_TH);            // [RF_C][ntop]
    const int64_t i = (int64_t)blockIdx.x * RF_TH + threadIdx.x;
    const int my_nan = rf_stage_features<RF_TH>(pl, F, n, i, feat);
    constexpr int NPRE = 12;  // RF_C * ntop <= 12 * RF_TH nodes per group (the host keeps ntop <= 3 * RF_TH)
    for (int c = 0; c < RF_C && c < n_trees; c++) {
        const rf_tree t0 = trees[c];
        const int cnt = t0.n_nodes < ntop ? t0.n_nodes : ntop;
        for (int j = threadIdx.x; j < cnt; j += RF_TH) top[(size_t)c * ntop + j] = nodes[t0.node_off + j];
    }
    const bool any_nan = __syncthreads_or(my_nan) != 0;
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.0;
    int n_oob = 0;
    const int n_groups = (n_trees + RF_C - 1) / RF_C;
    for (int g = 0; g < n_groups; g++) {
        const int t = g * RF_C;
        rf_tree tr[RF_C];
#pragma unroll
        for (int c = 0; c < RF_C; c++) tr[c] = trees[t + c < n_trees ? t + c : n_trees - 1];
        bool use[RF_C];
#pragma unroll
        for (int c = 0; c < RF_C; c++) {
            use[c] = t + c < n_trees && i < n;
            if (OOB) {
                const int cnt = use[c] ? o.counts[(size_t)(t + c) * (size_t)n + (size_t)i] : 1;
                use[c] = cnt == 0;
                n_oob += use[c] ? 1 : 0;
            }
        }
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
            for (int r = 0; r < NPRE; r++) {
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
                if (t + c >= n_trees || i >= n) nd[c].bits = RF_LEAF;  // no tree / no pixel: nothing to walk
            }
            if (any_nan) rf_walk_gen<true, RF_TH>(nd, lfeat, ltop, ntop, lim, nodes, noff);
            else rf_walk_gen<false, RF_TH>(nd, lfeat, ltop, ntop, lim, nodes, noff);
#pragma unroll
            for (int c = 0; c < RF_C; c++)
                if (use[c]) rf_vote<NC>(nd[c], leafval, acc);
        }
        if (more) {
            __syncthreads();  // every wave is done with the current blocks
#pragma unroll
            for (int r = 0; r < NPRE; r++) {
                const int j = threadIdx.x + r * RF_TH;
                if (j < RF_C * ntop) {
                    const int c = j / ntop, o2 = j - c * ntop;
                    int cnt = pcnt[0];
#pragma unroll
                    for (int cc = 1; cc < RF_C; cc++)
                        if (c == cc) cnt = pcnt[cc];
                    if (o2 < cnt) top[j] = pre[r];
                }
            }
            __syncthreads();
        }
    }
    if (i < n) rf_finish_out<NC, OOB>(acc, n_trees, n_oob, n_classes, classes, o, n, i);
}

// One launch of the loaded forest over n pixels into `o`, by the plan and the dispatch of k11_forest.h
template <bool OOB>
static int rf_launch_out(rsseg_ctx *ctx, const rf_planes &pl, int F, int64_t n, const rf_outputs &o, const char *prof_name)
{
    const rf_plan p = rf_launch_plan(ctx->forest, F);
    auto launch = [&](auto kern) { return rf_launch(ctx, p, prof_name, 1, kern, pl, F, n, rf_dev_classes(ctx->forest), o); };
    int rc = RSSEG_ERR_INVALID;
    if (p.lds_groups) { RF_DISPATCH(rc, p, launch, k11_forest_out_lds, OOB) }
    else { RF_DISPATCH(rc, p, launch, k11_forest_out_gen, OOB) }
    if (rc != RSSEG_OK) return rc;
    HIPCHK(ctx, hipGetLastError());
    return stream_sync(ctx);
}

extern "C" int rsseg_forest_predict_proba(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, double *d_proba, double *d_conf,
                                          int64_t *d_labels)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    rf_planes pl;
    RSCHK(rf_check_planes(ctx, "forest_predict_proba", d_planes, n >= 0, F, pl));
    if (!d_proba && !d_conf && !d_labels) return rs_fail(ctx, RSSEG_ERR_INVALID, "forest_predict_proba: every output is null");
    if (n == 0) return RSSEG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rf_outputs o;
    o.proba = d_proba;
    o.conf = d_conf;
    o.labels = (long long *)d_labels;
    o.counts = nullptr;
    o.n_oob = nullptr;
    return rf_launch_out<false>(ctx, pl, F, n, o, "forest_proba");
}

extern "C" int rsseg_forest_oob(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_counts, double *d_oob,
                                int32_t *d_n_oob)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    rf_planes pl;
    RSCHK(rf_check_planes(ctx, "forest_oob", d_planes, n >= 0, F, pl));
    if (!d_counts) return rs_fail(ctx, RSSEG_ERR_INVALID, "forest_oob: the bootstrap counts are null");
    if (!d_oob || !d_n_oob) return rs_fail(ctx, RSSEG_ERR_INVALID, "forest_oob: an output is null");
    if (n == 0) return RSSEG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rf_outputs o;
    o.proba = d_oob;
    o.conf = nullptr;
    o.labels = nullptr;
    o.counts = d_counts;
    o.n_oob = d_n_oob;
    return rf_launch_out<true>(ctx, pl, F, n, o, "forest_oob");
}
