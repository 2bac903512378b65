// K4 — GLCM texture windows for ANY list of (distance, angle) entries and up to 256 grey levels
// (graycomatrix(window, distances, angles, levels, symmetric=True, normed=True) + graycoprops(...).mean(), reference
// modules/features/indices.py:248-318, for any arguments the reference accepts).
//
// The host turns the entry list (offsets (dr, dc), rsseg/pipeline.py::glcm_offset_plan) into DISTINCT offsets: o and -o
// give the same symmetric matrix, and every offset that leaves the window gives the empty matrix.  One launch computes,
// for each window, the exact integer statistics of each distinct offset once (the names of k4_glcm.hip):
//     np, S1 = sum|a-b|, S2 = sum(a-b)^2, Hq = sum round(2^40/(1+(a-b)^2)), M1, M2, Mx,
//     A = sum_ij (G_ij+G_ji)^2 = 2 sum_cells c^2 + 2 sum_diagonal c^2   (c = count of an UNORDERED cell {a, b})
// and finishes each distinct offset in float64 with correctly rounded operations:
//     contrast S2/np, dissimilarity S1/np, homogeneity (Hq/np) 2^-40, energy sqrt(A)/(2 np), correlation glcm_corr;
//     np = 0 (the offset leaves the window) gives (0, 0, 0, 0, 1)
// then sums the ENTRIES left to right in entry order (an entry reads its distinct offset's values), divides by the
// entry count and rounds to float32.  tests/glcm_offsets_ref.py restates this bit for bit.
//
// The co-occurrence counts live in an LDS table of packed 16-bit counters over unordered cells, levels*(levels+1)/2 of
// them (a window of at most 255 x 255 has fewer than 2^16 pairs), cleared and reused per offset:
//   one WAVE per window for levels <= 64 (2080 cells, 4 KB; no workgroup barrier: a wave's LDS operations are ordered)
//   one WORKGROUP per window for 64 < levels <= 256 (32 896 cells, 64.3 KB of dynamic LDS)
// DEF: the four default angles at distance 1, finished over their common denominators with the 2^-52 sums of
// k4_glcm.hip (glcm_finish_hq): rsseg_glcm_u8 for 65..256 levels, equal to oracle.c mode 1.
#include <mutex>

#include "common.h"
#include "k4_glcm.h"

__constant__ long long c_glcmo_hq52[256];  // round(2^52 / (1 + d^2))
__constant__ long long c_glcmo_hq40[256];  // round(2^40 / (1 + d^2))

#define GLCMO_MAXK 64    // distinct offsets of one call
#define GLCMO_MAXN 512   // entries of one call

struct glcmo_plan {
    int K, n;
    int off[GLCMO_MAXK];               // distinct offsets: 16-bit dr (low half), 16-bit dc (high half)
    unsigned char idx[GLCMO_MAXN];     // entry -> distinct offset
};

template <bool WG> __device__ __forceinline__ void glcmo_sync()
{
    if constexpr (WG) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <bool WG, bool DEF>
__global__ __launch_bounds__(256) void k4_glcm_offsets(const uint8_t *__restrict__ q, int W, int levels, int win, int step, int oh,
                                                       int ow, glcm_out out, glcmo_plan plan, glcm_consts gc)
{
    extern __shared__ uint4 glcmo_lds[];
    __shared__ long long red[4][8];
    constexpr int NT = WG ? 256 : 64;
    const int ncell = levels * (levels + 1) / 2;
    const int tdw = ((ncell + 1) / 2 + 3) & ~3;          // table dwords (two counters each), a multiple of 4
    const int per = tdw + (DEF ? 0 : plan.K * 10);       // dwords per window: the table, then K x 5 doubles
    const int wave = threadIdx.x >> 6;
    const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    const long long widx = WG ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + wave;
    if (widx >= (long long)oh * ow) return;            // uniform over the window's threads
    unsigned *tab = reinterpret_cast<unsigned *>(glcmo_lds) + (WG ? 0 : wave * per);
    double *vals = reinterpret_cast<double *>(tab + tdw);
    const int oy = (int)(widx / ow), ox = (int)(widx - (long long)oy * ow);
    const uint8_t *wp = q + (size_t)oy * step * W + (size_t)ox * step;
    const int lmax = levels - 1;
    long long dst[4][7];       // DEF: per angle S1 S2 Hq.hi Hq.lo M1 M2 Mx
    long long dA[4];
    for (int k = 0; k < plan.K; k++) {
        const int o = plan.off[k];
        const int dr = (int)(short)(o & 0xffff), dc = (int)(short)((unsigned)o >> 16);
        const int adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
        const int np = (adr < win && adc < win) ? (win - adr) * (win - adc) : 0;
        long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // S1 S2 Hq.hi Hq.lo M1 M2 Mx A
        if (np > 0) {
            for (int i = tid * 4; i < tdw; i += NT * 4) *reinterpret_cast<uint4 *>(tab + i) = make_uint4(0, 0, 0, 0);
            glcmo_sync<WG>();
            const int r0 = dr < 0 ? -dr : 0, c0 = dc < 0 ? -dc : 0, pw = win - adc;
            int s1 = 0, s2 = 0, m1 = 0, m2 = 0, mx = 0;   // at most 1017 pairs per thread of at most 255^2 each
            long long hq = 0;                             // at most 1017 terms of at most 2^52
            for (int p = tid; p < np; p += NT) {
                const int rr = p / pw, r = r0 + rr, c = c0 + p - rr * pw;
                int x = wp[(size_t)r * W + c], y = wp[(size_t)(r + dr) * W + (c + dc)];
                x = x > lmax ? lmax : x;   // the quantiser guarantees < levels; never index outside the table
                y = y > lmax ? lmax : y;
                const int lo = x < y ? x : y, hi = x + y - lo;
                const int cell = lo * (2 * levels - lo + 1) / 2 + (hi - lo);
                atomicAdd(&tab[cell >> 1], 1u << (16 * (cell & 1)));
                const int d = hi - lo;
                s1 += d; s2 += d * d;
                hq += DEF ? c_glcmo_hq52[d] : c_glcmo_hq40[d];
                m1 += x + y; m2 += x * x + y * y; mx += 2 * x * y;
            }
            glcmo_sync<WG>();
            unsigned long long sq = 0;
            for (int i = tid; i < tdw; i += NT) {
                const unsigned v = tab[i], a = v & 0xffffu, b = v >> 16;
                sq += (unsigned long long)(a * a) + (unsigned long long)(b * b);
            }
            for (int l = tid; l < levels; l += NT) {
                const int cell = l * (2 * levels - l + 1) / 2;
                const unsigned c = (tab[cell >> 1] >> (16 * (cell & 1))) & 0xffffu;
                sq += (unsigned long long)(c * c);
            }
            const glcm_hq_sum hs = hq_split(hq);
            st[0] = s1; st[1] = s2; st[2] = hs.hi; st[3] = hs.lo; st[4] = m1; st[5] = m2; st[6] = mx; st[7] = 2 * (long long)sq;
#pragma unroll
            for (int t = 0; t < 8; t++) st[t] = wave_sum(st[t]);
            if constexpr (WG) {
                if ((threadIdx.x & 63) == 0) {
#pragma unroll
                    for (int t = 0; t < 8; t++) red[wave][t] = st[t];
                }
                __syncthreads();   // also: every read of the table is done before the next offset clears it
#pragma unroll
                for (int t = 0; t < 8; t++) st[t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
                __syncthreads();   // red is rewritten by the next offset
            } else {
                glcmo_sync<WG>();
            }
        }
        if constexpr (DEF) {
#pragma unroll
            for (int a = 0; a < 4; a++)
                if (a == k) {
#pragma unroll
                    for (int t = 0; t < 7; t++) dst[a][t] = st[t];
                    dA[a] = st[7];
                }
        } else if (tid == 0) {
            double *v = vals + 5 * k;
            if (np == 0) {
                v[0] = 0.0; v[1] = 0.0; v[2] = 0.0; v[3] = 0.0; v[4] = 1.0;
            } else {
                const double dn = (double)np;
                const long long Hq = (st[2] << GLCM_HQ_SPLIT) + st[3];   // below 2^56
                v[0] = (double)st[1] / dn;
                v[1] = (double)st[0] / dn;
                v[2] = ((double)Hq / dn) * (1.0 / 1099511627776.0);
                v[3] = sqrt((double)st[7]) / (double)(2 * (long long)np);
                v[4] = glcm_corr(np, st[4], st[5], st[6]);
            }
        }
    }
    if (tid != 0) return;
    const size_t o = (size_t)widx;
    if constexpr (DEF) {
        const long long na = (long long)win * (win - 1), nb = (long long)(win - 1) * (win - 1);
        glcm_group g0, g1;
        g0.S1 = dst[0][0] + dst[2][0]; g0.S2 = dst[0][1] + dst[2][1]; g0.Hq = 0;
        g0.sq = sqrt((double)dA[0]) + sqrt((double)dA[2]);
        g1.S1 = dst[1][0] + dst[3][0]; g1.S2 = dst[1][1] + dst[3][1]; g1.Hq = 0;
        g1.sq = sqrt((double)dA[1]) + sqrt((double)dA[3]);
        const double hq0 = hq_to_double(glcm_hq_sum{dst[0][2] + dst[2][2], dst[0][3] + dst[2][3]});
        const double hq1 = hq_to_double(glcm_hq_sum{dst[1][2] + dst[3][2], dst[1][3] + dst[3][3]});
        double r[4];
#pragma unroll
        for (int a = 0; a < 4; a++) r[a] = glcm_corr((a & 1) ? nb : na, dst[a][4], dst[a][5], dst[a][6]);
        glcm_finish_hq(g0, g1, hq0, hq1, na, nb, r[0], r[1], r[2], r[3], o, out, gc);
    } else {
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int e = 0; e < plan.n; e++) {
            const double *v = vals + 5 * plan.idx[e];
#pragma unroll
            for (int t = 0; t < 5; t++) s[t] += v[t];
        }
        const double dn = (double)plan.n;
#pragma unroll
        for (int t = 0; t < 5; t++)
            if (out.p[t]) out.p[t][o] = (float)(s[t] / dn);
    }
}

static bool g_hqo_ready[64] = {false};   // per device: the homogeneity tables are in place
static std::mutex g_hqo_mu;

int glcm_offsets_launch(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int levels, int win, int step, const int32_t *offsets, int n,
                        const glcm_out &out, bool def, const glcm_consts &gc)
{
    if (levels > 256 || win > 255)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: levels=%d win=%d: the unordered-cell kernels take levels <= 256 and win <= 255 "
                       "(16-bit counters)", levels, win);
    if (n > GLCMO_MAXN) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: %d (distance, angle) entries, at most %d supported", n, GLCMO_MAXN);
    glcmo_plan plan{};
    plan.n = n;
    for (int e = 0; e < n; e++) {
        long long dr = offsets[2 * e], dc = offsets[2 * e + 1];
        if (dr < 0 || (dr == 0 && dc < 0)) { dr = -dr; dc = -dc; }     // o and -o: the same symmetric matrix
        if (dr >= win || dc >= win || dc <= -win) { dr = win; dc = 0; } // every offset that leaves the window: the empty matrix
        const int o = (int)(((unsigned)dr & 0xffffu) | (((unsigned)dc & 0xffffu) << 16));
        int k = 0;
        while (k < plan.K && plan.off[k] != o) k++;
        if (k == plan.K) {
            if (plan.K == GLCMO_MAXK)
                return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: more than %d distinct offsets in one call", GLCMO_MAXK);
            plan.off[plan.K++] = o;
        }
        plan.idx[e] = (unsigned char)k;
    }
    if (def && plan.K != 4) return rs_fail(ctx, RSSEG_ERR_INVALID, "glcm: the default offsets are four distinct offsets");
    {
        std::lock_guard<std::mutex> g(g_hqo_mu);
        if (!g_hqo_ready[ctx->device & 63]) {
            long long l52[256], l40[256];
            for (int d = 0; d < 256; d++) {
                l52[d] = llrint(4503599627370496.0 / (1.0 + (double)d * (double)d));
                l40[d] = llrint(1099511627776.0 / (1.0 + (double)d * (double)d));
            }
            HIPCHK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_glcmo_hq52), l52, sizeof(l52)));
            HIPCHK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_glcmo_hq40), l40, sizeof(l40)));
            g_hqo_ready[ctx->device & 63] = true;
        }
    }
    const int oh = (H - win) / step + 1, ow = (W - win) / step + 1;
    const long long nwin = (long long)oh * ow;
    const int ncell = levels * (levels + 1) / 2;
    const size_t tdw = (size_t)(((ncell + 1) / 2 + 3) & ~3);
    const size_t per = (tdw + (def ? 0 : (size_t)plan.K * 10)) * 4;
    if (levels <= 64) {
        const void *kern = def ? (const void *)k4_glcm_offsets<false, true> : (const void *)k4_glcm_offsets<false, false>;
        RSCHK(set_max_dyn_lds(ctx, kern, 4 * per));
        const dim3 grid((unsigned)ceil_div64(nwin, 4));
        if (def) hipLaunchKernelGGL((k4_glcm_offsets<false, true>), grid, dim3(256), 4 * per, ctx->stream, d_q, W, levels, win, step, oh, ow, out, plan, gc);
        else hipLaunchKernelGGL((k4_glcm_offsets<false, false>), grid, dim3(256), 4 * per, ctx->stream, d_q, W, levels, win, step, oh, ow, out, plan, gc);
    } else {
        if (nwin > 2147483647ll) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: more than 2^31 - 1 windows for the workgroup-per-window kernel");
        const void *kern = def ? (const void *)k4_glcm_offsets<true, true> : (const void *)k4_glcm_offsets<true, false>;
        RSCHK(set_max_dyn_lds(ctx, kern, per));
        const dim3 grid((unsigned)nwin);
        if (def) hipLaunchKernelGGL((k4_glcm_offsets<true, true>), grid, dim3(256), per, ctx->stream, d_q, W, levels, win, step, oh, ow, out, plan, gc);
        else hipLaunchKernelGGL((k4_glcm_offsets<true, false>), grid, dim3(256), per, ctx->stream, d_q, W, levels, win, step, oh, ow, out, plan, gc);
    }
    HIPCHK(ctx, hipGetLastError());
    return RSSEG_OK;
}

extern "C" int rsseg_glcm_offsets_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int levels, int win, int step,
                                     const int32_t *offsets, int n, float *const *d_props)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_q || !d_props || !offsets || n < 1 || H < 1 || W < 1 || levels < 2 || win < 2 || win > H || win > W || step < 1)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "glcm: bad arguments (H=%d W=%d levels=%d win=%d step=%d n=%d)", H, W, levels, win, step, n);
    static const int32_t def[8] = {0, 1, 1, 1, 1, 0, 1, -1};
    if (n == 4 && !memcmp(offsets, def, sizeof(def))) return rsseg_glcm_u8(ctx, d_q, H, W, levels, win, step, d_props);
    if (levels > 256)   // the quantised plane is uint8; NumPy's astype(uint8) of values above 255 is platform-defined
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: levels=%d > 256 not supported (the quantised plane is uint8)", levels);
    if (win > 255)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: window %d > 255 with non-default offsets (16-bit co-occurrence counters)", win);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    glcm_out out;
    for (int i = 0; i < 5; i++) out.p[i] = d_props[i];
    {
        prof_scope ps(ctx, "glcm");
        RSCHK(glcm_offsets_launch(ctx, d_q, H, W, levels, win, step, offsets, n, out, false, glcm_consts{}));
    }
    return stream_sync(ctx);
}
