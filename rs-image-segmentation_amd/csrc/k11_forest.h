// K11 — the node layout, the vote rows and the walks shared by the forest kernels (k11_forest.hip: labels;
// k11_forest_proba.hip: class probabilities, confidence and the out-of-bag sums).  The layout is described at the
// top of k11_forest.hip, where rsseg_forest_load builds it.
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

struct rf_group {   // k11_forest_lds: trees [first, first + count) whose nodes [node_base, node_base + n_nodes) share the LDS
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

// ---- k11_forest_lds ------------------------------------------------------------------------------------------------
// A thread owns RF_PX pixels of its workgroup's 1024 and walks RF_C trees for each: RF_PX * RF_C independent chains.
// One round advances every chain by one node: all feature reads back to back, all node reads back to back, no control
// flow (leaves are fixed points).  Lanes leave the loop when all their chains sit on leaves.
#define RF_PX 1                      // pixels per thread (k11_forest_lds): TH threads per workgroup
#define RF_NCH (RF_PX * RF_C)

template <bool NANS>
__device__ __forceinline__ void rf_round_lds(rf_node (&nd)[RF_NCH], unsigned feat_tid, unsigned px_stride, const unsigned (&base)[RF_C])
{
    // feat_tid: LDS address of the thread's first pixel's feature row ([pixel][FP] floats, FP odd: conflict-free fills)
    float x[RF_NCH];
#pragma unroll
    for (int q = 0; q < RF_NCH; q++)   // chain q: pixel q / RF_C of the thread, tree q % RF_C of the group
        x[q] = *RF_LDS_PTR(lds_cfloat, feat_tid + (q / RF_C) * px_stride + (nd[q].bits >> 24));
#pragma unroll
    for (int q = 0; q < RF_NCH; q++) {
        bool go_right = x[q] > nd[q].thr;
        if (NANS) go_right = go_right || (x[q] != x[q] && !(nd[q].bits & RF_MISS));
        const unsigned next = (nd[q].bits & RF_CHILD) + (go_right ? 1u : 0u);
        lds_cnode *p = RF_LDS_PTR(lds_cnode, base[q % RF_C] + next * 8u);
        nd[q].thr = p->thr;
        nd[q].bits = p->bits;
    }
}

// Leaves are fixed points, so for deep forests (`two`: the host sets it from the deepest tree) the exit test runs every
// SECOND round: one test costs as much as a chain step, and a lane that reaches its last leaf after an odd number of
// rounds merely repeats it once.  Shallow forests (the reference's bundled model: depth <= 5) keep the test every round.
template <bool NANS>
__device__ __forceinline__ void rf_walk_lds(rf_node (&nd)[RF_NCH], unsigned feat_tid, unsigned px_stride, const unsigned (&base)[RF_C], bool two)
{
    for (;;) {
        unsigned all = nd[0].bits;
#pragma unroll
        for (int q = 1; q < RF_NCH; q++) all &= nd[q].bits;
        if (all & RF_LEAF) break;
        rf_round_lds<NANS>(nd, feat_tid, px_stride, base);
        if (two) rf_round_lds<NANS>(nd, feat_tid, px_stride, base);
    }
}

#define RF_NPRE (6 * RF_PX)   // 16-byte pieces (2 nodes) a thread prefetches per group: cap <= 12 * 1024 nodes

// ---- k11_forest_gen ------------------------------------------------------------------------------------------------
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

// pixels per workgroup: 1024 while the feature rows and the vote accumulators allow it
static int rf_threads(int F, int n_classes) { return (F <= 32 && n_classes <= 32) ? 1024 : 512; }
// nodes of a tree group that fit the LDS beside the features of TH pixels (one 16-byte piece is kept for the dummy leaf)
static int rf_lds_cap(int F, int TH)
{
    const long bytes = 160L * 1024 - 256 - (long)(F | 1) * TH * 4 - 16;
    long cap = bytes / 8;
    cap = std::min<long>(cap, 2L * RF_NPRE * (TH / RF_PX)) & ~1L;
    return (int)std::max<long>(cap, 0);
}
