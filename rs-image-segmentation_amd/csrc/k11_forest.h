// K11 — what the forest kernels share: the node layout, the vote rows, the walks, the prefetch registers of the LDS-group
// kernels and the host-side launch path (launch plan, dispatch over (row width, threads), launch, plane checks).
// k11_forest.hip (labels), k11_forest_proba.hip (class probabilities, confidence, out-of-bag sums) and k11_forest_perm.hip
// (permutation counts) each hold their LDS-group and their general kernel written out: as policies on shared
// __forceinline__ bodies the kernels computed the same values but did not keep the parent's registers and speed (DESIGN.md
// section 5).  The layout is described at the top of k11_forest.hip, where rsseg_forest_load builds it.
#pragma once
#include <algorithm>

#include "common.h"

struct __align__(8) rf_node {
    float thr;
    unsigned bits;
};
// bits: [0,22) index of the left child within the tree (right = left + 1; a leaf: its own index), bit 22 missing-goes-
// left, bit 23 leaf, byte 3 = 4 * feature (0 on a leaf).  Byte 3 is a clean byte offset into a pixel's feature row, so
// the walk forms the feature address with ONE instruction (v_add_u32 with a byte-3 operand select) instead of
// shift + mask + add, and the child index needs one mask.
#define RF_LEAF 0x00800000u
#define RF_MISS 0x00400000u
#define RF_CHILD 0x003fffffu
#define RF_NAN_BITS 0x7fc00000u   // leaf thr: quiet NaN | payload
#define RF_PAY_MASK 0x003fffffu   // payload: row of the vote table

#define RF_NCMAX 64
static_assert(RSSEG_MAX_FEATURES <= 64, "byte 3 of a node holds 4 * feature");
#define RF_C 4        // trees walked at a time (independent chains of dependent LDS reads)

struct rf_planes {
    const float *p[RSSEG_MAX_FEATURES];
};

struct rf_tree {
    int node_off;  // first node of the tree in the node array
    int n_nodes;
    int leaf_off;  // first row of the tree in the leaf-value table
    int pad;
};

struct rf_group {   // LDS-group kernels: trees [first, first + count) whose nodes [node_base, node_base + n_nodes) share the LDS
    int first, count;
    int node_base;  // even (16-byte aligned copy); <= node_off of the first tree
    int n_nodes;    // nodes copied (from node_base)
};

typedef __attribute__((address_space(3))) const float lds_cfloat;
typedef __attribute__((address_space(3))) const rf_node lds_cnode;
// an LDS address is 32 bits wide on the device; the host pass of the same source sees 64-bit pointers and would warn
#if defined(__HIP_DEVICE_COMPILE__)
#define RF_LDS_PTR(T, a) ((T *)(a))
#else
#define RF_LDS_PTR(T, a) ((T *)(uintptr_t)(a))
#endif

// The vote of a leaf: its row of the table, added in tree order (x + 0.0 == x, so a one-hot row adds a single 1.0).
template <int NC>
__device__ __forceinline__ void rf_row_load(const rf_node nd, const double *__restrict__ leafval, double (&row)[NC])
{
    const double2 *v = reinterpret_cast<const double2 *>(leafval + (size_t)(__float_as_uint(nd.thr) & RF_PAY_MASK) * NC);
#pragma unroll
    for (int c = 0; c < NC / 2; c++) {
        const double2 t = v[c];
        row[2 * c] = t.x;
        row[2 * c + 1] = t.y;
    }
}
template <int NC>
__device__ __forceinline__ void rf_vote(const rf_node nd, const double *__restrict__ leafval, double (&acc)[NC])
{
    double row[NC];
    rf_row_load<NC>(nd, leafval, row);
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] += row[c];
}

// rf_vote in pieces of 8 doubles.  The accumulators of the widest rows take half the registers a lane may have (NC = 32 at
// 1024 threads: 64 of 128; NC = 64 at 512: 128 of 256), and a whole row loaded beside them goes to scratch memory; the
// compiler barrier keeps the pieces apart.  One addition per class and tree, in tree order, as rf_vote: the same sums.
template <int NC>
__device__ __forceinline__ void rf_vote_pieces(const rf_node nd, const double *__restrict__ leafval, double (&acc)[NC])
{
    const double2 *v = reinterpret_cast<const double2 *>(leafval + (size_t)(__float_as_uint(nd.thr) & RF_PAY_MASK) * NC);
    constexpr int P = NC / 2 < 4 ? NC / 2 : 4;   // double2 per piece
#pragma unroll
    for (int c0 = 0; c0 < NC / 2; c0 += P) {
        double2 t[P];
#pragma unroll
        for (int k = 0; k < P; k++) t[k] = v[c0 + k];
#pragma unroll
        for (int k = 0; k < P; k++) {
            acc[2 * (c0 + k)] += t[k].x;
            acc[2 * (c0 + k) + 1] += t[k].y;
        }
        if (NC > 16) asm volatile("" ::: "memory");
    }
}

// the general kernels stage the pixel's own row as [F][TH] floats (bank = lane); returns whether a value is NaN
template <int TH>
__device__ __forceinline__ int rf_stage_features(const rf_planes &pl, int F, int64_t n, int64_t i, float *feat)
{
    int my_nan = 0;
    for (int f = 0; f < F; f++) {
        const float v = i < n ? pl.p[f][i] : 0.f;
        my_nan |= v != v;
        feat[f * TH + threadIdx.x] = v;
    }
    return my_nan;
}

// ---- the LDS-group kernels: walk and prefetch registers -----------------------------------------------------------------
// A thread owns one pixel of its workgroup's RF_TH and walks RF_C trees for it: RF_C independent chains.
// One round advances every chain by one node: all feature reads back to back, all node reads back to back, no control
// flow (leaves are fixed points).  Lanes leave the loop when all their chains sit on leaves.
template <bool NANS>
__device__ __forceinline__ void rf_round_lds(rf_node (&nd)[RF_C], unsigned feat_tid, const unsigned (&base)[RF_C])
{
    // feat_tid: LDS address of the thread's pixel's feature row ([pixel][FP] floats, FP odd: conflict-free fills)
    float x[RF_C];
#pragma unroll
    for (int q = 0; q < RF_C; q++)   // chain q: tree q of the group
        x[q] = *RF_LDS_PTR(lds_cfloat, feat_tid + (nd[q].bits >> 24));
#pragma unroll
    for (int q = 0; q < RF_C; q++) {
        bool go_right = x[q] > nd[q].thr;
        if (NANS) go_right = go_right || (x[q] != x[q] && !(nd[q].bits & RF_MISS));
        const unsigned next = (nd[q].bits & RF_CHILD) + (go_right ? 1u : 0u);
        lds_cnode *p = RF_LDS_PTR(lds_cnode, base[q] + next * 8u);
        nd[q].thr = p->thr;
        nd[q].bits = p->bits;
    }
}

// Leaves are fixed points, so for deep forests (`two`: the host sets it from the deepest tree) the exit test runs every
// SECOND round: one test costs as much as a chain step, and a lane that reaches its last leaf after an odd number of
// rounds merely repeats it once.  Shallow forests (the reference's bundled model: depth <= 5) keep the test every round.
template <bool NANS>
__device__ __forceinline__ void rf_walk_lds(rf_node (&nd)[RF_C], unsigned feat_tid, const unsigned (&base)[RF_C], bool two)
{
    for (;;) {
        unsigned all = nd[0].bits;
#pragma unroll
        for (int q = 1; q < RF_C; q++) all &= nd[q].bits;
        if (all & RF_LEAF) break;
        rf_round_lds<NANS>(nd, feat_tid, base);
        if (two) rf_round_lds<NANS>(nd, feat_tid, base);
    }
}

#define RF_NPRE 6   // 16-byte pieces (2 nodes) a thread prefetches per group: cap <= 12 * RF_TH nodes
// The prefetch of the next group (one contiguous range, 16-byte loads, held in registers during the walk) and the refill
// behind the barrier, register r of RF_NPRE; they read psrc, plast, npiece, top and RF_TH of the kernel that uses them.
// Six named registers, not an array: the compiler kept `uint4 pre[6]` in scratch memory across the walk (96 bytes per lane
// written and read back per group = 800 B/px of HBM traffic: profiles/r02_c5_pmc_traffic.md, first r02 set)
#define RF_PRE(r) const uint4 pre##r = psrc[(int)threadIdx.x + r * RF_TH < plast ? (int)threadIdx.x + r * RF_TH : plast];
#define RF_PUT(r) if ((int)threadIdx.x + r * RF_TH < npiece) top[threadIdx.x + r * RF_TH] = pre##r;

// ---- the general kernels: the walk --------------------------------------------------------------------------------------
// Any forest: the first ntop (breadth-first) nodes of each of RF_C trees in LDS, deeper nodes by global loads.
// Every load of a round is issued unconditionally (a chain on its leaf reads node 0 of its block and keeps its leaf by a
// select): a load inside a per-chain `if` makes the compiler wait for each LDS read before it issues the next one,
// which serialises the chains.  Only a step to a node beyond the LDS block takes a predicated global load.
template <bool NANS, int RF_TH>
__device__ __forceinline__ void rf_walk_gen(rf_node (&nd)[RF_C], lds_cfloat *feat, lds_cnode *top, int ntop, const int (&lim)[RF_C],
                                            const rf_node *__restrict__ nodes, const int (&noff)[RF_C])
{
    for (;;) {
        unsigned all = 0xffffffffu;
#pragma unroll
        for (int c = 0; c < RF_C; c++) all &= nd[c].bits;
        if (all & RF_LEAF) break;   // every chain of this lane sits on a leaf (lanes leave the loop one by one)
        float x[RF_C];
        unsigned leafm[RF_C];  // all ones when the chain sits on its leaf (bit 31 of the node), as a mask: no control flow
#pragma unroll
        for (int c = 0; c < RF_C; c++) {
            leafm[c] = (unsigned)((int)(nd[c].bits << 8) >> 31);
            const unsigned f4 = nd[c].bits >> 24;          // 4 * feature; 0 on a leaf
            x[c] = feat[f4 * (RF_TH / 4) + threadIdx.x];
        }
        unsigned next[RF_C], out[RF_C];
        rf_node ld[RF_C];
#pragma unroll
        for (int c = 0; c < RF_C; c++) {
            bool go_right = x[c] > nd[c].thr;
            if (NANS) go_right = go_right || (x[c] != x[c] && !(nd[c].bits & RF_MISS));
            next[c] = (nd[c].bits & RF_CHILD) + (go_right ? 1u : 0u);
            out[c] = ((int)next[c] >= lim[c] ? 0xffffffffu : 0u) & ~leafm[c];
            const unsigned a = next[c] & ~(leafm[c] | out[c]);
            lds_cnode *p = top + c * ntop + a;
            ld[c].thr = p->thr;
            ld[c].bits = p->bits;
        }
#pragma unroll
        for (int c = 0; c < RF_C; c++) {
            nd[c].thr = leafm[c] ? nd[c].thr : ld[c].thr;
            nd[c].bits = leafm[c] ? nd[c].bits : ld[c].bits;
        }
        if (out[0] | out[1] | out[2] | out[3]) {
#pragma unroll
            for (int c = 0; c < RF_C; c++)
                if (out[c]) nd[c] = nodes[noff[c] + next[c]];
        }
    }
}

// ---- the host side: one launch path for the four entry points ---------------------------------------------------------
// pixels per workgroup: 1024 while the feature rows and the vote accumulators allow it
static int rf_threads(int F, int n_classes) { return (F <= 32 && n_classes <= 32) ? 1024 : 512; }
// nodes of a tree group that fit the LDS beside the features of TH pixels (one 16-byte piece is kept for the dummy leaf)
static int rf_lds_cap(int F, int TH)
{
    const long bytes = 160L * 1024 - 256 - (long)(F | 1) * TH * 4 - 16;
    long cap = bytes / 8;
    cap = std::min<long>(cap, 2L * RF_NPRE * TH) & ~1L;
    return (int)std::max<long>(cap, 0);
}
// row length of the vote table: n_classes padded with zeros
static int rf_row_width(int n_classes) { return n_classes <= 4 ? 4 : (n_classes <= 8 ? 8 : (n_classes <= 16 ? 16 : (n_classes <= 32 ? 32 : 64))); }

// the checks the entry points share (each under its own name `who`); fills `pl`
static int rf_check_planes(rsseg_ctx *ctx, const char *who, const float *const *d_planes, bool args_ok, int F, rf_planes &pl)
{
    forest_dev &fd = ctx->forest;
    if (!fd.d_nodes) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: no forest loaded", who);
    if (!d_planes || !args_ok) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: bad arguments", who);
    if (F != fd.n_features)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: X has %d features, but the forest is expecting %d features as input", who, F, fd.n_features);
    memset(&pl, 0, sizeof(pl));
    for (int f = 0; f < F; f++) {
        if (!d_planes[f]) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: plane %d is null", who, f);
        pl.p[f] = d_planes[f];
    }
    return RSSEG_OK;
}

struct rf_plan {
    int TH, NC;        // threads (= pixels) per workgroup, row length of the vote table
    bool lds_groups;   // rsseg_forest_load found a plan: the LDS-group kernel; otherwise the general one
    int cap;           // LDS-group: nodes of the node area
    int ntop;          // general: nodes per tree held in LDS
    size_t lds;        // dynamic LDS bytes
};
// the launch plan of the loaded forest for F features
static rf_plan rf_launch_plan(const forest_dev &fd, int F)
{
    rf_plan p;
    p.TH = rf_threads(F, fd.n_classes);
    p.NC = rf_row_width(fd.n_classes);
    p.lds_groups = fd.n_groups > 0;
    // every group of trees fits the LDS: features TH * (F | 1) * 4 B + cap nodes + the dummy leaf
    p.cap = rf_lds_cap(F, p.TH);
    // a tree larger than the LDS area: the first ntop (breadth-first) nodes of RF_C trees in LDS, in steps of 256
    p.ntop = 3 * p.TH;
    while (p.ntop > 256 && (size_t)F * p.TH * 4 + (size_t)RF_C * p.ntop * sizeof(rf_node) > 158 * 1024) p.ntop -= 256;
    p.lds = p.lds_groups ? (size_t)(F | 1) * p.TH * 4 + (size_t)p.cap * sizeof(rf_node) + 16
                         : (size_t)F * p.TH * 4 + (size_t)RF_C * p.ntop * sizeof(rf_node);
    return p;
}

// the (row width, threads) pairs: 1024 threads up to 32 classes, 512 for every width.  KERN: a kernel template over
// <NC, RF_TH> and whatever template arguments follow; `launch(kernel)` returns a status
#define RF_DISPATCH(rc, plan, launch, KERN, ...)                                         \
    if ((plan).TH == 1024) {                                                             \
        if ((plan).NC == 4) rc = launch(KERN<4, 1024, ##__VA_ARGS__>);                   \
        else if ((plan).NC == 8) rc = launch(KERN<8, 1024, ##__VA_ARGS__>);              \
        else if ((plan).NC == 16) rc = launch(KERN<16, 1024, ##__VA_ARGS__>);            \
        else rc = launch(KERN<32, 1024, ##__VA_ARGS__>);                                 \
    } else {                                                                             \
        if ((plan).NC == 4) rc = launch(KERN<4, 512, ##__VA_ARGS__>);                    \
        else if ((plan).NC == 8) rc = launch(KERN<8, 512, ##__VA_ARGS__>);               \
        else if ((plan).NC == 16) rc = launch(KERN<16, 512, ##__VA_ARGS__>);             \
        else if ((plan).NC == 32) rc = launch(KERN<32, 512, ##__VA_ARGS__>);             \
        else rc = launch(KERN<64, 512, ##__VA_ARGS__>);                                  \
    }

template <class T>
struct rf_as_is {
    typedef T type;
};
// One launch of the loaded forest over n pixels and grid_y jobs.  The two overloads are told apart by the kernel's own
// argument list; `tail` is what the kernel takes behind n_classes.
template <class... Tail>
static int rf_launch(rsseg_ctx *ctx, const rf_plan &p, const char *prof_name, unsigned grid_y,
                     void (*kern)(rf_planes, int, int64_t, const rf_node *, const rf_tree *, const rf_group *, int, int, int, int, const double *, int, Tail...),
                     const rf_planes &pl, int F, int64_t n, typename rf_as_is<Tail>::type... tail)
{
    forest_dev &fd = ctx->forest;
    const rf_tree *d_trees = (const rf_tree *)((const char *)fd.d_treeoff + fd.n_classes * sizeof(long long));
    RSCHK(set_max_dyn_lds(ctx, (const void *)kern, p.lds));
    prof_scope ps(ctx, prof_name);
    hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div64(n, p.TH), grid_y), dim3(p.TH), p.lds, ctx->stream, pl, F, n, (const rf_node *)fd.d_nodes,
                       d_trees, (const rf_group *)fd.d_groups, fd.n_groups, p.cap / 2, fd.max_depth >= 10 ? 1 : 0, fd.n_trees,
                       (const double *)fd.d_leafval, fd.n_classes, tail...);
    return RSSEG_OK;
}
template <class... Tail>
static int rf_launch(rsseg_ctx *ctx, const rf_plan &p, const char *prof_name, unsigned grid_y,
                     void (*kern)(rf_planes, int, int64_t, const rf_node *, const rf_tree *, int, int, const double *, int, Tail...),
                     const rf_planes &pl, int F, int64_t n, typename rf_as_is<Tail>::type... tail)
{
    forest_dev &fd = ctx->forest;
    const rf_tree *d_trees = (const rf_tree *)((const char *)fd.d_treeoff + fd.n_classes * sizeof(long long));
    RSCHK(set_max_dyn_lds(ctx, (const void *)kern, p.lds));
    prof_scope ps(ctx, prof_name);
    hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div64(n, p.TH), grid_y), dim3(p.TH), p.lds, ctx->stream, pl, F, n, (const rf_node *)fd.d_nodes,
                       d_trees, fd.n_trees, p.ntop, (const double *)fd.d_leafval, fd.n_classes, tail...);
    return RSSEG_OK;
}
// the classes (int64) sit in front of the per-tree records
static const long long *rf_dev_classes(const forest_dev &fd) { return (const long long *)fd.d_treeoff; }
