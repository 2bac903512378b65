// K17 — 2-D correlation of a uint8 plane with a bank of float32 kernels of one odd size (cv2.filter2D's direct path:
// centre anchor, BORDER_REFLECT_101, float32), the filter bank of calculate_gabor_features (indices.py:346-399).
//
// Contract: out[f][y][x] = sum over i, then j, of k[f][i][j] * u8[y + i - m][x + j - m], m = ksize / 2, started
// from +0, every product and every sum ONE float32 operation (the build's -ffp-contract=off), subnormals kept.  A uint8 sample
// is non-negative and the sum starts at +0, so a zero tap's +-0 product leaves the sum's bits alone: no branch on it.
//
// A 256-thread workgroup owns a tile of K17_TW x K17_TH outputs:
//   1. the (K17_TH + 2m) x (K17_TW + 2m) input tile is staged in LDS once, widened to float32 (exact), the border rule
//      applied while staging; byte loads, so any W and any alignment;
//   2. a thread owns K17_RUN = 4 adjacent columns and K17_RPT rows.  For an output row it walks the K tile rows top to bottom;
//      of each it reads the 4 + 2m values under its run (ds_read_b128) and slides them under the K taps of that row for all
//      NF kernels of the launch: one LDS value feeds up to NF x 4 multiply-adds, the NF x 4 independent sums supply the
//      instruction-level parallelism, and per sum the order is rows outer, columns inner;
//   3. the taps are laid out [i][j][NF] in a small device buffer every lane reads at the same address (scalar loads: the
//      NF taps of one (i, j) are one s_load_dwordx8 at NF = 8);
//   4. the extrema of every plane are reduced in the same pass: wave reduction, one commit per workgroup into one of
//      RSSEG_MM_REPL replica lines of ordered keys (mm_key / mm_unkey, as k8_filter does).
// All orientations of a scale share ksize and the staged tile, so one launch computes up to K17_MAXF of them.
// The normalised form writes the raw planes, reads the extrema back and divides in place (k17_normalise): 8 B/px per plane
// against ~2 * ksize^2 VALU operations per pixel and plane for a recomputing second pass.
// Whole plane, single device: there is no rows= / sharded form of this operator.
#include <cmath>
#include <type_traits>

#include "border.h"
#include "common.h"

#define K17_TW 128                     // output columns per workgroup
#define K17_TH 32                      // output rows per workgroup
#define K17_RUN 4                      // adjacent columns per thread
#define K17_RPT 4                      // output rows per thread
#define K17_MAXK 15                    // largest kernel size
#define K17_MAXF 8                     // kernels per launch
#define K17_SGPR_TAPS 32               // taps requested together (scalar registers)
#define K17_TSTRIDE (K17_TW + 16)      // floats per tile row: 128 + 2 * 7 rounded up to whole 16-byte reads
static_assert(K17_TW / K17_RUN * (K17_TH / K17_RPT) == 256, "one thread per run of the tile");
static_assert(K17_MAXF * 2 <= 16, "a replica line of 16 keys holds every plane's {min, max}");

struct k17_planes {
    float *out[K17_MAXF];
};

// taps: [K][K][NF] (kernels beyond nf are all zero and are not written).  mm: [RSSEG_MM_REPL][16] ordered keys, {min, max} of
// plane f at 2f.
template <int K, int NF>
__global__ __launch_bounds__(256) void k17_correlate(const uint8_t *__restrict__ q, int H, int W, const float *__restrict__ taps, k17_planes pl, int nf,
                                                     uint32_t *__restrict__ mm)
{
    constexpr int M = K / 2, NR = K17_TH + 2 * M, NC = K17_TW + 2 * M, NV = (K17_RUN + 2 * M + 3) / 4;
    __shared__ __align__(16) float tile[NR * K17_TSTRIDE];
    const int x0 = blockIdx.x * K17_TW, y0 = blockIdx.y * K17_TH;
    // tile row r holds input row reflect(y0 - M + r), tile column c input column reflect(x0 - M + c); positions further than M
    // outside the plane are under no output of the plane and are left zero
    for (int s = threadIdx.x; s < NR * K17_TSTRIDE; s += 256) {
        const int r = s / K17_TSTRIDE, c = s - r * K17_TSTRIDE;
        const int gy = y0 - M + r, gx = x0 - M + c;
        float v = 0.f;
        if (c < NC && gy < H + M && gx < W + M)
            v = (float)q[(size_t)border_idx(gy, H, BORDER_REFLECT_101) * W + border_idx(gx, W, BORDER_REFLECT_101)];
        tile[s] = v;
    }
    __syncthreads();

    const int cx = (threadIdx.x & 31) * K17_RUN, ry = (threadIdx.x >> 5) * K17_RPT;
    float lmn[NF], lmx[NF];
#pragma unroll
    for (int f = 0; f < NF; f++) { lmn[f] = INFINITY; lmx[f] = -INFINITY; }
    const bool vec = (W & 3) == 0;   // with the planes 16-byte aligned (checked by the host)
    if (x0 + cx < W) {
        for (int rr = 0; rr < K17_RPT; rr++) {
            const int row = ry + rr, oy = y0 + row;
            if (oy >= H) break;
            float acc[NF][K17_RUN];
#pragma unroll
            for (int f = 0; f < NF; f++)
#pragma unroll
                for (int r = 0; r < K17_RUN; r++) acc[f][r] = 0.f;
#pragma unroll 1
            for (int i = 0; i < K; i++) {
                float w[4 * NV];
                const float4 *src = reinterpret_cast<const float4 *>(tile + (row + i) * K17_TSTRIDE + cx);
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    const float4 a = src[v];
                    w[4 * v] = a.x; w[4 * v + 1] = a.y; w[4 * v + 2] = a.z; w[4 * v + 3] = a.w;
                }
                const float *__restrict__ t = taps + i * (K * NF);
#pragma unroll
                for (int j = 0; j < K; j++) {
                    // a row's K * NF taps do not fit the scalar registers beside the rest: without a fence the scheduler
                    // requests them all at once and parks the overflow in vector-register lanes
                    if (K * NF > K17_SGPR_TAPS && j > 0 && j % (K17_SGPR_TAPS / NF) == 0) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int f = 0; f < NF; f++) {
                        const float tf = t[j * NF + f];
#pragma unroll
                        for (int r = 0; r < K17_RUN; r++) {
                            const float p = tf * w[j + r];
                            acc[f][r] = acc[f][r] + p;
                        }
                    }
                }
            }
            const size_t o = (size_t)oy * W + (x0 + cx);
#pragma unroll
            for (int f = 0; f < NF; f++) {
                if (f < nf) {
                    float *p = pl.out[f] + o;
                    if (vec) *reinterpret_cast<float4 *>(p) = make_float4(acc[f][0], acc[f][1], acc[f][2], acc[f][3]);
#pragma unroll
                    for (int r = 0; r < K17_RUN; r++)
                        if (x0 + cx + r < W) {
                            if (!vec) p[r] = acc[f][r];
                            lmn[f] = fminf(lmn[f], acc[f][r]);
                            lmx[f] = fmaxf(lmx[f], acc[f][r]);
                        }
                }
            }
        }
    }
    // one commit per workgroup and plane; lanes without pixels carry +inf / -inf and never win
    __shared__ float smn[4][NF], smx[4][NF];
#pragma unroll
    for (int f = 0; f < NF; f++) {
        const float a = wave_min(lmn[f]), b = wave_max(lmx[f]);
        if (lane_id() == 0) { smn[threadIdx.x >> 6][f] = a; smx[threadIdx.x >> 6][f] = b; }
    }
    __syncthreads();
    if ((int)threadIdx.x < nf) {
        const int f = threadIdx.x;
        const float mn = fminf(fminf(smn[0][f], smn[1][f]), fminf(smn[2][f], smn[3][f])), mx = fmaxf(fmaxf(smx[0][f], smx[1][f]), fmaxf(smx[2][f], smx[3][f]));
        const uint32_t kmn = mm_key(mn), kmx = mm_key(mx);
        uint32_t *rs = mm + 16 * ((blockIdx.y * gridDim.x + blockIdx.x) % RSSEG_MM_REPL) + 2 * f;
        if (kmn < __builtin_nontemporal_load(&rs[0])) atomicMin(&rs[0], kmn);
        if (kmx > __builtin_nontemporal_load(&rs[1])) atomicMax(&rs[1], kmx);
    }
}

// (r - min) / den in place, plane blockIdx.y; a true division.  16-byte accesses where the plane starts aligned (every plane
// does when H * W is a multiple of 4)
struct k17_norm {
    float sub[K17_MAXF], den[K17_MAXF];
};
__global__ __launch_bounds__(256) void k17_normalise(k17_planes pl, k17_norm nm, int64_t n)
{
    float *__restrict__ p = pl.out[blockIdx.y];
    const float sub = nm.sub[blockIdx.y], den = nm.den[blockIdx.y];
    const int64_t n4 = ((uintptr_t)p & 15) == 0 ? n >> 2 : 0;
    // two independent 16-byte accesses per thread, both requested before either is used
    const int64_t i0 = (int64_t)blockIdx.x * (2 * 256) + threadIdx.x, i1 = i0 + 256;
    float4 a, b;
    if (i0 < n4) a = reinterpret_cast<const float4 *>(p)[i0];
    if (i1 < n4) b = reinterpret_cast<const float4 *>(p)[i1];
    if (i0 < n4) {
        a.x = (a.x - sub) / den; a.y = (a.y - sub) / den; a.z = (a.z - sub) / den; a.w = (a.w - sub) / den;
        reinterpret_cast<float4 *>(p)[i0] = a;
    }
    if (i1 < n4) {
        b.x = (b.x - sub) / den; b.y = (b.y - sub) / den; b.z = (b.z - sub) / den; b.w = (b.w - sub) / den;
        reinterpret_cast<float4 *>(p)[i1] = b;
    }
    // what the 16-byte accesses leave: the last n % 4 elements, or all of a plane that does not start aligned
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = (p[i] - sub) / den;
}

template <int K> static void launch_k(int nft, dim3 grid, hipStream_t s, const uint8_t *q, int H, int W, const float *taps, const k17_planes &pl, int nf, uint32_t *mm)
{
    switch (nft) {
    case 1: hipLaunchKernelGGL((k17_correlate<K, 1>), grid, dim3(256), 0, s, q, H, W, taps, pl, nf, mm); break;
    case 2: hipLaunchKernelGGL((k17_correlate<K, 2>), grid, dim3(256), 0, s, q, H, W, taps, pl, nf, mm); break;
    case 4: hipLaunchKernelGGL((k17_correlate<K, 4>), grid, dim3(256), 0, s, q, H, W, taps, pl, nf, mm); break;
    case 6: hipLaunchKernelGGL((k17_correlate<K, 6>), grid, dim3(256), 0, s, q, H, W, taps, pl, nf, mm); break;
    default: hipLaunchKernelGGL((k17_correlate<K, 8>), grid, dim3(256), 0, s, q, H, W, taps, pl, nf, mm); break;
    }
}
// kernels a launch is compiled for: the smallest of {1, 2, 4, 6, 8} that holds nf
static int k17_width(int nf) { return nf <= 2 ? nf : (nf <= 4 ? 4 : (nf <= 6 ? 6 : 8)); }

extern "C" void rsseg_correlate_tile(int *tile_h, int *tile_w)
{
    if (tile_h) *tile_h = K17_TH;
    if (tile_w) *tile_w = K17_TW;
}

// raw responses of all nf kernels, K17_MAXF per launch, and their extrema; `norm`: the in-place normalising pass after each launch
static int correlate(rsseg_ctx *ctx, const char *what, const uint8_t *d_q, int H, int W, const float *h_taps, int ksize, int nf, float *d_out,
                     float *h_minmax, bool norm)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (ksize < 1 || ksize > K17_MAXK || !(ksize & 1)) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: kernel size %d is not odd and within 1..%d", what, ksize, K17_MAXK);
    if (nf < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: %d kernels (at least 1)", what, nf);
    if (H < 1 || W < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: a %d x %d plane", what, H, W);
    if (!d_q || !h_taps || !d_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: bad arguments", what);
    if ((const void *)d_q == (const void *)d_out) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: in-place not supported", what);
    if ((uintptr_t)d_out & 15) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: the output is not 16-byte aligned", what);
    const int kk = ksize * ksize;
    for (int64_t i = 0; i < (int64_t)nf * kk; i++)
        if (!std::isfinite(h_taps[i])) return rs_fail(ctx, RSSEG_ERR_INVALID, "%s: tap %lld of kernel %lld is not finite", what, (long long)(i % kk), (long long)(i / kk));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t key_bytes = 64 * RSSEG_MM_REPL, tap_bytes = sizeof(float) * K17_MAXK * K17_MAXK * K17_MAXF;
    RSCHK(ws_reserve(ctx, key_bytes + tap_bytes));
    RSCHK(pin_reserve(ctx, key_bytes + tap_bytes));
    uint32_t *d_keys = (uint32_t *)ctx->d_ws;
    float *d_taps = (float *)(ctx->d_ws + key_bytes), *h_pin_taps = (float *)(ctx->h_pin + key_bytes);
    const uint32_t *h_keys = (const uint32_t *)ctx->h_pin;
    const size_t n = (size_t)H * W;
    const dim3 grid((W + K17_TW - 1) / K17_TW, (H + K17_TH - 1) / K17_TH);
    for (int f0 = 0; f0 < nf; f0 += K17_MAXF) {
        const int g = std::min(nf - f0, K17_MAXF), nft = k17_width(g);
        for (int t = 0; t < kk; t++)
            for (int f = 0; f < nft; f++) h_pin_taps[t * nft + f] = f < g ? h_taps[(size_t)(f0 + f) * kk + t] : 0.f;
        k17_planes pl;
        memset(&pl, 0, sizeof(pl));
        for (int f = 0; f < g; f++) pl.out[f] = d_out + (size_t)(f0 + f) * n;
        HIPCHK(ctx, hipMemcpyAsync(d_taps, h_pin_taps, sizeof(float) * kk * nft, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_keys, 0, key_bytes, ctx->stream));
        for (int f = 0; f < g; f++) HIPCHK(ctx, hipMemset2DAsync(d_keys + 2 * f, 64, 0xff, 4, RSSEG_MM_REPL, ctx->stream));
        {
            prof_scope ps(ctx, "correlate");
            switch (ksize) {
            case 1: launch_k<1>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            case 3: launch_k<3>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            case 5: launch_k<5>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            case 7: launch_k<7>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            case 9: launch_k<9>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            case 11: launch_k<11>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            case 13: launch_k<13>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            default: launch_k<15>(nft, grid, ctx->stream, d_q, H, W, d_taps, pl, g, d_keys); break;
            }
        }
        HIPCHK(ctx, hipGetLastError());
        // always read back: the wait also frees the pinned tap buffer for the next launch
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_keys, key_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, rs_sync(ctx));
        k17_norm nm;
        memset(&nm, 0, sizeof(nm));
        for (int f = 0; f < g; f++) {
            uint32_t kmn = 0xffffffffu, kmx = 0;
            for (int r = 0; r < RSSEG_MM_REPL; r++) {
                kmn = std::min(kmn, h_keys[16 * r + 2 * f]);
                kmx = std::max(kmx, h_keys[16 * r + 2 * f + 1]);
            }
            const float mn = mm_unkey(kmn), mx = mm_unkey(kmx);
            if (h_minmax) { h_minmax[2 * (f0 + f)] = mn; h_minmax[2 * (f0 + f) + 1] = mx; }
            nm.sub[f] = mn;
            nm.den[f] = norm_den(mn, mx);   // fl(fl(max - min) + 1e-10f), as filter_rows<1>
        }
        if (norm) {
            prof_scope ps(ctx, "correlate_norm");
            const int64_t blocks = std::max<int64_t>(((int64_t)n + 2047) / 2048, 1);   // 2 x 256 x 4 elements per workgroup
            hipLaunchKernelGGL(k17_normalise, dim3((unsigned)blocks, g), dim3(256), 0, ctx->stream, pl, nm, (int64_t)n);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    return norm ? stream_sync(ctx) : RSSEG_OK;
}

extern "C" int rsseg_correlate_u8_f32(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, const float *h_taps, int ksize, int nf, float *d_out,
                                      float *h_minmax)
{
    return correlate(ctx, "correlate", d_q, H, W, h_taps, ksize, nf, d_out, h_minmax, false);
}

extern "C" int rsseg_filter_bank_norm_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, const float *h_taps, int ksize, int nf, float *d_out)
{
    return correlate(ctx, "filter_bank_norm", d_q, H, W, h_taps, ksize, nf, d_out, nullptr, true);
}
