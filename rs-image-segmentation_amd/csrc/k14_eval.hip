// K14 — joint count table of (truth value, predicted value) over the pixels where truth > 0: the one pass every metric of
// the reference's accuracy assessment derives from (confusion_matrix, accuracy_score, cohen_kappa_score,
// classification_report and the cluster -> class majority mapping of scripts/4_evaluate.py:72-160 and
// modules/evaluation.py:32-63).
//
// Two passes over the two integer planes, each HBM-bound (6 B/px for an int16 truth and an int32 prediction):
//   k14_label_range  the number of valid pixels, min / max of truth and of pred over them (one partial per workgroup,
//                    reduced on the host: no initialised device state, no atomics);
//   k14_confusion    the dense table, cell (t - tmin) * np + (p - pmin), in LDS uint32 counters with several private
//                    copies per workgroup (the pattern of k1_hist_u8), flushed with 64-bit integer atomics into an int64
//                    table: integer sums do not depend on arrival order, so the result is deterministic.
// Both read 16 bytes per lane per plane and instruction, grid-stride; workgroup 0 takes the tail that is not a whole chunk.

#include "common.h"

#include <climits>

#define EV_THREADS 1024
#define EV_GRID 512            // the two 1024-thread workgroups per CU that are resident anyway (as K1's 256-bin pass)
#define EV_MAX_CELLS 4096
#define EV_LDS_WORDS 16384     // 64 KB of counters per workgroup at most
#define EV_MAX_COPIES 64

// pixels per chunk: one 16-byte load of the narrower plane, as many as needed of the wider one
template <typename TT, typename TP>
struct ev_chunk {
    static constexpr int E = 16 / (sizeof(TT) < sizeof(TP) ? sizeof(TT) : sizeof(TP));
};

template <typename T, int E>
__device__ __forceinline__ void ev_load(const T *__restrict__ x, int64_t c, T (&out)[E])
{
    constexpr int NV = E * (int)sizeof(T) / 16;
    const rs_u4v *src = reinterpret_cast<const rs_u4v *>(x) + c * NV;
    union {
        rs_u4v u[NV];
        T t[E];
    } b;
#pragma unroll
    for (int k = 0; k < NV; k++) b.u[k] = __builtin_nontemporal_load(src + k);
#pragma unroll
    for (int e = 0; e < E; e++) out[e] = b.t[e];
}

__device__ __forceinline__ long long ev_wave_min(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
    return v;
}
__device__ __forceinline__ long long ev_wave_max(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

// part[blockIdx.x][5] = {valid count, tmin, tmax, pmin, pmax}; a workgroup without valid pixels writes (0, +inf, -inf, +inf, -inf)
template <typename TT, typename TP>
__global__ __launch_bounds__(EV_THREADS) void k14_label_range(const TT *__restrict__ truth, const TP *__restrict__ pred, int64_t n,
                                                              long long *__restrict__ part)
{
    constexpr int E = ev_chunk<TT, TP>::E;
    long long cnt = 0, tmn = LLONG_MAX, tmx = LLONG_MIN, pmn = LLONG_MAX, pmx = LLONG_MIN;
    auto take = [&](TT t, TP p) {
        if (t > TT(0)) {
            const long long tv = (long long)t, pv = (long long)p;
            cnt++;
            tmn = tv < tmn ? tv : tmn;
            tmx = tv > tmx ? tv : tmx;
            pmn = pv < pmn ? pv : pmn;
            pmx = pv > pmx ? pv : pmx;
        }
    };
    const int64_t nch = n / E, stride = (int64_t)gridDim.x * EV_THREADS;
    for (int64_t c = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; c < nch; c += stride) {
        TT t[E];
        TP p[E];
        ev_load<TT, E>(truth, c, t);
        ev_load<TP, E>(pred, c, p);
#pragma unroll
        for (int e = 0; e < E; e++) take(t[e], p[e]);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nch * E + threadIdx.x; i < n; i += EV_THREADS) take(truth[i], pred[i]);
    __shared__ long long s[EV_THREADS / 64][5];
    cnt = wave_sum(cnt);
    tmn = ev_wave_min(tmn);
    tmx = ev_wave_max(tmx);
    pmn = ev_wave_min(pmn);
    pmx = ev_wave_max(pmx);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { s[w][0] = cnt; s[w][1] = tmn; s[w][2] = tmx; s[w][3] = pmn; s[w][4] = pmx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < EV_THREADS / 64; i++) {
            cnt += s[i][0];
            tmn = s[i][1] < tmn ? s[i][1] : tmn;
            tmx = s[i][2] > tmx ? s[i][2] : tmx;
            pmn = s[i][3] < pmn ? s[i][3] : pmn;
            pmx = s[i][4] > pmx ? s[i][4] : pmx;
        }
        long long *o = part + (size_t)blockIdx.x * 5;
        o[0] = cnt; o[1] = tmn; o[2] = tmx; o[3] = pmn; o[4] = pmx;
    }
}

// table[nt * np] += counts, table[nt * np] (one past the table) += valid pixels outside [tmin, tmin + nt) x [pmin, pmin + np)
// (possible only with a caller-supplied range).  Dynamic LDS: copies x stride uint32, stride = (nt * np) | 1 (odd, so that
// the copies of one cell fall in different banks); a lane adds into copy (threadIdx.x & (copies - 1)).
template <typename TT, typename TP>
__global__ __launch_bounds__(EV_THREADS) void k14_confusion(const TT *__restrict__ truth, const TP *__restrict__ pred, int64_t n,
                                                            long long tmin, long long pmin, uint32_t nt, uint32_t np,
                                                            uint32_t stride_w, uint32_t copies, unsigned long long *__restrict__ table)
{
    constexpr int E = ev_chunk<TT, TP>::E;
    extern __shared__ uint32_t lt[];
    const uint32_t cells = nt * np;
    for (uint32_t i = threadIdx.x; i < copies * stride_w; i += EV_THREADS) lt[i] = 0;
    __syncthreads();
    uint32_t *mine = lt + (threadIdx.x & (copies - 1)) * stride_w;
    uint32_t outside = 0;
    // unsigned differences: a value below the range wraps to a large number and fails the bound test like one above it
    auto take = [&](TT t, TP p) {
        if (t > TT(0)) {
            const uint64_t ti = (uint64_t)(long long)t - (uint64_t)tmin, pi = (uint64_t)(long long)p - (uint64_t)pmin;
            if (ti < nt && pi < np)
                atomicAdd(&mine[(uint32_t)ti * np + (uint32_t)pi], 1u);
            else
                outside++;
        }
    };
    const int64_t nch = n / E, stride = (int64_t)gridDim.x * EV_THREADS;
    for (int64_t c = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; c < nch; c += stride) {
        TT t[E];
        TP p[E];
        ev_load<TT, E>(truth, c, t);
        ev_load<TP, E>(pred, c, p);
#pragma unroll
        for (int e = 0; e < E; e++) take(t[e], p[e]);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nch * E + threadIdx.x; i < n; i += EV_THREADS) take(truth[i], pred[i]);
    outside = wave_sum(outside);
    if (lane_id() == 0 && outside) atomicAdd(&table[cells], (unsigned long long)outside);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < cells; c += EV_THREADS) {
        uint32_t s = 0;
        for (uint32_t cp = 0; cp < copies; cp++) s += lt[cp * stride_w + c];
        if (s) atomicAdd(&table[c], (unsigned long long)s);
    }
}

namespace {

struct ev_launch {
    rsseg_ctx *ctx;
    const void *truth, *pred;
    int64_t n;
    int grid;
};

// the two passes for one (truth, pred) dtype pair
template <typename TT, typename TP>
struct ev_pair {
    static int range(const ev_launch &L, long long *d_part)
    {
        prof_scope ps(L.ctx, "eval_range");
        hipLaunchKernelGGL((k14_label_range<TT, TP>), dim3(L.grid), dim3(EV_THREADS), 0, L.ctx->stream, (const TT *)L.truth,
                           (const TP *)L.pred, L.n, d_part);
        HIPCHK(L.ctx, hipGetLastError());
        return RSSEG_OK;
    }
    static int table(const ev_launch &L, long long tmin, long long pmin, uint32_t nt, uint32_t np, uint32_t stride_w, uint32_t copies,
                     unsigned long long *d_table)
    {
        const size_t lds = (size_t)copies * stride_w * 4;
        RSCHK(set_max_dyn_lds(L.ctx, (const void *)k14_confusion<TT, TP>, lds));
        prof_scope ps(L.ctx, "eval_table");
        hipLaunchKernelGGL((k14_confusion<TT, TP>), dim3(L.grid), dim3(EV_THREADS), lds, L.ctx->stream, (const TT *)L.truth,
                           (const TP *)L.pred, L.n, tmin, pmin, nt, np, stride_w, copies, d_table);
        HIPCHK(L.ctx, hipGetLastError());
        return RSSEG_OK;
    }
};

template <typename TT>
int ev_dispatch_pred(int pred_dtype, bool range_pass, const ev_launch &L, long long *d_part, long long tmin, long long pmin, uint32_t nt,
                     uint32_t np, uint32_t stride_w, uint32_t copies, unsigned long long *d_table)
{
#define EV_GO(TP) \
    return range_pass ? ev_pair<TT, TP>::range(L, d_part) : ev_pair<TT, TP>::table(L, tmin, pmin, nt, np, stride_w, copies, d_table)
    switch (pred_dtype) {
    case RSSEG_U8: EV_GO(uint8_t);
    case RSSEG_I32: EV_GO(int32_t);
    case RSSEG_I64: EV_GO(int64_t);
    }
#undef EV_GO
    return RSSEG_ERR_INVALID;
}

int ev_dispatch(int truth_dtype, int pred_dtype, bool range_pass, const ev_launch &L, long long *d_part, long long tmin = 0,
                long long pmin = 0, uint32_t nt = 0, uint32_t np = 0, uint32_t stride_w = 0, uint32_t copies = 0,
                unsigned long long *d_table = nullptr)
{
#define EV_T(TT) return ev_dispatch_pred<TT>(pred_dtype, range_pass, L, d_part, tmin, pmin, nt, np, stride_w, copies, d_table)
    switch (truth_dtype) {
    case RSSEG_U8: EV_T(uint8_t);
    case RSSEG_I16: EV_T(int16_t);
    case RSSEG_U16: EV_T(uint16_t);
    case RSSEG_I32: EV_T(int32_t);
    case RSSEG_I64: EV_T(int64_t);
    }
#undef EV_T
    return RSSEG_ERR_INVALID;
}

size_t ev_size(int dtype)
{
    switch (dtype) {
    case RSSEG_U8: return 1;
    case RSSEG_I16:
    case RSSEG_U16: return 2;
    case RSSEG_I32: return 4;
    case RSSEG_I64: return 8;
    }
    return 0;
}

}  // namespace

extern "C" int rsseg_confusion_counts(rsseg_ctx *ctx, const void *d_truth, int truth_dtype, const void *d_pred, int pred_dtype,
                                      int64_t n_local, const int64_t *known_range, int64_t range_out[4], int64_t *n_valid,
                                      int64_t *counts, int64_t cap)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    const size_t tsz = ev_size(truth_dtype), psz = ev_size(pred_dtype);
    if (!tsz || !(pred_dtype == RSSEG_U8 || pred_dtype == RSSEG_I32 || pred_dtype == RSSEG_I64))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "confusion_counts: truth dtype %d / prediction dtype %d not supported", truth_dtype, pred_dtype);
    if (n_local < 0 || !range_out || !n_valid || cap < 0 || (cap > 0 && !counts))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "confusion_counts: bad arguments (n=%lld cap=%lld)", (long long)n_local, (long long)cap);
    if (n_local > 0 && (!d_truth || !d_pred || ((uintptr_t)d_truth & 15) != 0 || ((uintptr_t)d_pred & 15) != 0))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "confusion_counts: planes must be non-null and 16-byte aligned");
    if (n_local >= (1LL << 40))   // a workgroup's uint32 counters hold n_local / EV_GRID pixels at most
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "confusion_counts: %lld pixels per rank exceed 2^40", (long long)n_local);
    if (known_range && (known_range[0] > known_range[1] || known_range[2] > known_range[3]))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "confusion_counts: known_range {%lld, %lld, %lld, %lld} is empty",
                       (long long)known_range[0], (long long)known_range[1], (long long)known_range[2], (long long)known_range[3]);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t nch = n_local / (int64_t)(16 / std::min(tsz, psz));
    const int grid = (int)std::min<int64_t>(EV_GRID, std::max<int64_t>(1, ceil_div64(nch, EV_THREADS)));
    const ev_launch L{ctx, d_truth, d_pred, n_local, grid};
    const size_t part_bytes = (size_t)EV_GRID * 5 * 8, table_bytes = (size_t)(EV_MAX_CELLS + 1) * 8;
    RSCHK(ws_reserve(ctx, part_bytes + table_bytes));
    RSCHK(pin_reserve(ctx, std::max(part_bytes, table_bytes)));
    long long *d_part = (long long *)ctx->d_ws;
    unsigned long long *d_table = (unsigned long long *)(ctx->d_ws + part_bytes);
    long long *h = (long long *)ctx->h_pin;

    long long tmin, tmax, pmin, pmax, nv = -1;
    if (known_range) {
        tmin = known_range[0]; tmax = known_range[1]; pmin = known_range[2]; pmax = known_range[3];
    } else {
        // pass 1: the ranges; then SUM of the count, MIN of {tmin, pmin}, MAX of {tmax, pmax} across ranks
        long long r[5] = {0, LLONG_MAX, LLONG_MIN, LLONG_MAX, LLONG_MIN};
        if (n_local > 0) {
            RSCHK(ev_dispatch(truth_dtype, pred_dtype, true, L, d_part));
            HIPCHK(ctx, hipMemcpyAsync(h, d_part, (size_t)grid * 5 * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, rs_sync(ctx));
            for (int b = 0; b < grid; b++) {
                const long long *q = h + (size_t)b * 5;
                r[0] += q[0];
                r[1] = std::min(r[1], q[1]);
                r[2] = std::max(r[2], q[2]);
                r[3] = std::min(r[3], q[3]);
                r[4] = std::max(r[4], q[4]);
            }
        }
        long long mn[2] = {r[1], r[3]}, mx[2] = {r[2], r[4]};
        RSCHK(comm_allreduce_host(ctx, &r[0], 1, RSSEG_I64, RSSEG_SUM));
        RSCHK(comm_allreduce_host(ctx, mn, 2, RSSEG_I64, RSSEG_MIN));
        RSCHK(comm_allreduce_host(ctx, mx, 2, RSSEG_I64, RSSEG_MAX));
        nv = r[0];
        *n_valid = nv;
        if (nv == 0) {   // no valid pixel on any rank: empty ranges, no table
            range_out[0] = 0; range_out[1] = -1; range_out[2] = 0; range_out[3] = -1;
            return RSSEG_OK;
        }
        tmin = mn[0]; pmin = mn[1]; tmax = mx[0]; pmax = mx[1];
    }
    range_out[0] = tmin; range_out[1] = tmax; range_out[2] = pmin; range_out[3] = pmax;
    // extents without overflow: the differences of ordered int64 values fit in uint64
    const uint64_t dt = (uint64_t)tmax - (uint64_t)tmin, dp = (uint64_t)pmax - (uint64_t)pmin;
    const uint64_t lim = (uint64_t)std::min<int64_t>(cap, EV_MAX_CELLS);
    if (dt >= lim || dp >= lim || (dt + 1) * (dp + 1) > lim) {
        if (nv < 0) *n_valid = -1;
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "confusion_counts: truth %lld..%lld x prediction %lld..%lld exceeds %llu cells",
                       tmin, tmax, pmin, pmax, (unsigned long long)lim);
    }
    const uint32_t nt = (uint32_t)dt + 1, np = (uint32_t)dp + 1, cells = nt * np;
    const uint32_t stride_w = cells | 1u;
    uint32_t copies = EV_MAX_COPIES;
    while (copies > 1 && copies * stride_w > EV_LDS_WORDS) copies >>= 1;

    // pass 2: the table (+ the outside counter), one SUM across ranks
    HIPCHK(ctx, hipMemsetAsync(d_table, 0, (size_t)(cells + 1) * 8, ctx->stream));
    if (n_local > 0) RSCHK(ev_dispatch(truth_dtype, pred_dtype, false, L, nullptr, tmin, pmin, nt, np, stride_w, copies, d_table));
    HIPCHK(ctx, hipMemcpyAsync(h, d_table, (size_t)(cells + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    RSCHK(comm_allreduce_host(ctx, h, (int64_t)cells + 1, RSSEG_I64, RSSEG_SUM));
    if (h[cells] != 0)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "confusion_counts: %lld valid pixels lie outside known_range {%lld, %lld, %lld, %lld}",
                       h[cells], tmin, tmax, pmin, pmax);
    long long total = 0;
    for (uint32_t c = 0; c < cells; c++) {
        counts[c] = h[c];
        total += h[c];
    }
    *n_valid = total;
    return RSSEG_OK;
}
