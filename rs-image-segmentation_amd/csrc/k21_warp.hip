// K21 — geometric correction: a multi-band polynomial resampling gather.  The host (rsseg/georect.py) fits the ground
// control points and composes the backward polynomial with the output grid; the kernel evaluates, per output pixel (r, c),
//   X = (c + 0.5) - cx,  Y = (r + 0.5) - cy
//   u = ((((p0 + p1*X) + p2*Y) + p3*(X*X)) + p4*(X*Y)) + p5*(Y*Y)      v likewise from q0..q5
// in double, one IEEE operation per written operation (the Makefile sets -ffp-contract=off; no fma is called), and samples
// every source plane at (u, v) (pixel-corner coordinates: the first pixel's centre is (0.5, 0.5)) with nearest, bilinear
// or cubic-convolution (Keys, a = -0.5) weights, edge-replicated taps.  A pixel with !(0 <= u < W && 0 <= v < H) (NaN
// included) gets `fill` and mask 0, and its coordinates are never converted to integers.  tests/warp_ref.py restates
// the arithmetic in NumPy operation for operation; the kernel is bit-equal to it.
//
// One 256-thread workgroup owns a tile of 4 output rows by 64 threads; a thread owns one pixel, or for nearest with a 1- or
// 2-byte output PX = 4 / sizeof(output element) adjacent pixels of one row, which it stores as one dword (warp_px).  Per
// pixel the coordinates, validity, tap indices and weights are computed once and kept in registers across the loop over
// the bands; all taps of a band are loaded before they are combined, without a branch around the loads.  Tiles are walked
// grid-stride, so the valid count costs one atomic per wave.

#include "common.h"

#include <cmath>
#include <type_traits>

#define WARP_THREADS 256
#define WARP_ROWS 4          // rows of a tile (one wave each)
#define WARP_MAX_BANDS 16    // PRE_MAX_BANDS of k15_preprocess.hip
#define WARP_WG_TARGET 8192  // 256 CUs x 8 workgroups x 4: the grid's cap; the tiles beyond it are walked grid-stride

#define WARP_NEAREST 0
#define WARP_BILINEAR 1
#define WARP_CUBIC 2

struct warp_args {
    const void *in[WARP_MAX_BANDS];
    void *out[WARP_MAX_BANDS];
    uint8_t *mask;               // or null
    unsigned long long *count;   // valid pixels (zeroed before the launch)
    double p[6], q[6], cx, cy, fill;
    int H, W, Ho, Wo, nb;
};

// a dword store at an element-aligned address (an odd output width, or a plane that starts at an odd element of its
// allocation): global memory takes it at any alignment, the type only tells the compiler so
typedef uint32_t warp_u32_any __attribute__((aligned(1)));
typedef uint16_t warp_u16_any __attribute__((aligned(1)));

__device__ __forceinline__ int warp_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Keys' cubic convolution weights, a = -0.5, for a tap at distance t: near |t| <= 1, far 1 <= |t| <= 2
__device__ __forceinline__ double warp_keys_near(double t)
{
    const double t2 = t * t, t3 = t2 * t;
    return (1.5 * t3 - 2.5 * t2) + 1.0;
}
__device__ __forceinline__ double warp_keys_far(double t)
{
    const double t2 = t * t, t3 = t2 * t;
    return ((-0.5 * t3 + 2.5 * t2) - 4.0 * t) + 2.0;
}

// what a thread keeps per pixel across the band loop
template <int M> struct warp_state;
template <> struct warp_state<WARP_NEAREST> {
    int64_t off;
    __device__ __forceinline__ void set(double u, double v, int H, int W)
    {
        const double fx = u - 0.5, fy = v - 0.5;
        const int x = warp_clampi((int)floor(fx + 0.5), W - 1), y = warp_clampi((int)floor(fy + 0.5), H - 1);
        off = (int64_t)y * W + x;
    }
};
template <> struct warp_state<WARP_BILINEAR> {
    int64_t r0, r1;
    int x0, x1;
    double tx, ty;
    __device__ __forceinline__ void set(double u, double v, int H, int W)
    {
        const double fx = u - 0.5, fy = v - 0.5;
        const double bx = floor(fx), by = floor(fy);
        tx = fx - bx;
        ty = fy - by;
        const int ix = (int)bx, iy = (int)by;   // -1 ... W - 1, -1 ... H - 1
        x0 = warp_clampi(ix, W - 1);
        x1 = warp_clampi(ix + 1, W - 1);
        r0 = (int64_t)warp_clampi(iy, H - 1) * W;
        r1 = (int64_t)warp_clampi(iy + 1, H - 1) * W;
    }
};
template <> struct warp_state<WARP_CUBIC> {
    int64_t ro[4];
    int xo[4];
    double wx[4], wy[4];
    __device__ __forceinline__ void set(double u, double v, int H, int W)
    {
        const double fx = u - 0.5, fy = v - 0.5;
        const double bx = floor(fx), by = floor(fy);
        const double tx = fx - bx, ty = fy - by;
        const int ix = (int)bx, iy = (int)by;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            xo[i] = warp_clampi(ix - 1 + i, W - 1);
            ro[i] = (int64_t)warp_clampi(iy - 1 + i, H - 1) * W;
        }
        // taps i = -1, 0, 1, 2 lie at |t - i| = t + 1, t, 1 - t, 2 - t
        wx[0] = warp_keys_far(tx + 1.0);
        wx[1] = warp_keys_near(tx);
        wx[2] = warp_keys_near(1.0 - tx);
        wx[3] = warp_keys_far(2.0 - tx);
        wy[0] = warp_keys_far(ty + 1.0);
        wy[1] = warp_keys_near(ty);
        wy[2] = warp_keys_near(1.0 - ty);
        wy[3] = warp_keys_far(2.0 - ty);
    }
};

// double -> the output element: integers round half to even and saturate, float32 is one cast
template <typename To> __device__ __forceinline__ To warp_finish(double v)
{
    if constexpr (std::is_integral<To>::value) {
        const double lo = (double)std::numeric_limits<To>::lowest(), hi = (double)std::numeric_limits<To>::max();
        double r = rint(v);
        r = r < lo ? lo : r;
        r = r > hi ? hi : r;
        return (To)r;
    } else {
        return (To)v;
    }
}

template <typename T, typename To, int M>
__device__ __forceinline__ To warp_sample(const T *__restrict__ src, const warp_state<M> &s)
{
    if constexpr (M == WARP_NEAREST) {
        return (To)src[s.off];   // T == To: the value's bits as they are
    } else if constexpr (M == WARP_BILINEAR) {
        const T g00 = src[s.r0 + s.x0], g01 = src[s.r0 + s.x1], g10 = src[s.r1 + s.x0], g11 = src[s.r1 + s.x1];
        const double ux = 1.0 - s.tx;
        const double top = (double)g00 * ux + (double)g01 * s.tx;
        const double bot = (double)g10 * ux + (double)g11 * s.tx;
        return warp_finish<To>(top * (1.0 - s.ty) + bot * s.ty);
    } else {
        T g[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) g[j][i] = src[s.ro[j] + s.xo[i]];
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double row = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++) row = row + s.wx[i] * (double)g[j][i];
            acc = acc + s.wy[j] * row;
        }
        return warp_finish<To>(acc);
    }
}

// pixels per thread: a 1- or 2-byte nearest output packs 4 or 2 results into one dword store (measured 3.1 ms against 3.6 ms
// with byte stores, 7 uint8 bands at 16384^2).  Not for bilinear and cubic: four pixels' fractions, offsets and taps cost
// 116 VGPRs (bilinear, uint8) and more for cubic, a wave or more per SIMD, and bilinear measured 8.9 ms against 5.4 ms with
// one pixel per thread (profiles/warp_variants_ab.json, profiles/warp_code_objects.json)
__host__ __device__ constexpr int warp_px(size_t out_size, int method) { return out_size < 4 && method == WARP_NEAREST ? 4 / (int)out_size : 1; }

template <typename To> struct warp_word { typedef To U; };
template <> struct warp_word<int16_t> { typedef uint16_t U; };

template <typename T, typename To, int M>
__global__ __launch_bounds__(WARP_THREADS) void k21_warp(const warp_args a, int64_t tiles, int tiles_x)
{
    constexpr int PX = warp_px(sizeof(To), M);
    constexpr int EB = 8 * (int)sizeof(To);   // bits of an output element
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const To fill = (To)a.fill;   // the host has checked that the type holds it
    unsigned nvalid = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t trow = t / tiles_x;
        const int tcol = (int)(t - trow * tiles_x);
        const int64_t r = trow * WARP_ROWS + ly, c0 = ((int64_t)tcol * 64 + lx) * PX;
        if (r >= a.Ho || c0 >= a.Wo) continue;
        const int64_t o0 = r * a.Wo + c0;   // < 2^39
        const int npx = a.Wo - c0 < PX ? (int)(a.Wo - c0) : PX;
        const double Y = ((double)r + 0.5) - a.cy;
        // the state of the thread's PX pixels, then the bands: every tap of a band's PX pixels is loaded before any is combined.
        // An invalid pixel reads the source's first pixel and drops the result (no branch around the loads); its own
        // coordinates are never converted.  A pixel past the row's end repeats the row's last one and is not stored.
        warp_state<M> s[PX];
        uint32_t mbits = 0;
#pragma unroll
        for (int p = 0; p < PX; p++) {
            const double X = ((double)(c0 + (p < npx ? p : npx - 1)) + 0.5) - a.cx;
            const double XX = X * X, XY = X * Y, YY = Y * Y;
            const double u = ((((a.p[0] + a.p[1] * X) + a.p[2] * Y) + a.p[3] * XX) + a.p[4] * XY) + a.p[5] * YY;
            const double v = ((((a.q[0] + a.q[1] * X) + a.q[2] * Y) + a.q[3] * XX) + a.q[4] * XY) + a.q[5] * YY;
            const bool ok = p < npx && u >= 0.0 && u < (double)a.W && v >= 0.0 && v < (double)a.H;   // false for NaN
            s[p].set(ok ? u : 0.5, ok ? v : 0.5, a.H, a.W);
            mbits |= (ok ? 1u : 0u) << (8 * p);
        }
        nvalid += __builtin_popcount(mbits);
#pragma unroll
        for (int b = 0; b < WARP_MAX_BANDS; b++) {
            if (b < a.nb) {
                const T *src = (const T *)a.in[b];
                To val[PX];
#pragma unroll
                for (int p = 0; p < PX; p++) val[p] = warp_sample<T, To, M>(src, s[p]);
#pragma unroll
                for (int p = 0; p < PX; p++) val[p] = (mbits >> (8 * p) & 1u) ? val[p] : fill;
                To *o = (To *)a.out[b] + o0;
                if constexpr (PX == 1) {
                    o[0] = val[0];
                } else if (npx == PX) {
                    uint32_t word = 0;
#pragma unroll
                    for (int p = 0; p < PX; p++) word |= (uint32_t)(typename warp_word<To>::U)val[p] << (EB * p);
                    *reinterpret_cast<warp_u32_any *>(o) = word;
                } else {
#pragma unroll
                    for (int p = 0; p < PX; p++)
                        if (p < npx) o[p] = val[p];
                }
            }
        }
        if (a.mask) {
            uint8_t *m = a.mask + o0;
            if (PX == 4 && npx == 4) *reinterpret_cast<warp_u32_any *>(m) = mbits;
            else if (PX == 2 && npx == 2) *reinterpret_cast<warp_u16_any *>(m) = (uint16_t)mbits;
            else
                for (int p = 0; p < npx; p++) m[p] = (uint8_t)(mbits >> (8 * p) & 1u);
        }
    }
    // one atomic per wave
    unsigned long long tot = wave_sum((unsigned long long)nvalid);
    if (lane_id() == 0 && tot) atomicAdd(a.count, tot);
}

namespace {

const char *warp_dtype_name(int dtype)
{
    switch (dtype) {
    case RSSEG_F32: return "float32";
    case RSSEG_F64: return "float64";
    case RSSEG_I64: return "int64";
    case RSSEG_U8: return "uint8";
    case RSSEG_I16: return "int16";
    case RSSEG_U16: return "uint16";
    case RSSEG_I32: return "int32";
    }
    return "unknown";
}

size_t warp_size(int dtype)
{
    switch (dtype) {
    case RSSEG_U8: return 1;
    case RSSEG_I16:
    case RSSEG_U16: return 2;
    case RSSEG_I32:
    case RSSEG_F32: return 4;
    case RSSEG_F64: return 8;
    }
    return 0;   // RSSEG_I64 and anything else
}

// the integer range of an output dtype (false: a float type, which holds any fill)
bool warp_int_range(int dtype, double *lo, double *hi)
{
    switch (dtype) {
    case RSSEG_U8: *lo = 0; *hi = 255; return true;
    case RSSEG_I16: *lo = -32768; *hi = 32767; return true;
    case RSSEG_U16: *lo = 0; *hi = 65535; return true;
    case RSSEG_I32: *lo = -2147483648.0; *hi = 2147483647.0; return true;
    }
    return false;
}

template <typename T, typename To>
void warp_launch(rsseg_ctx *ctx, int method, const warp_args &a, unsigned grid, int64_t tiles, int tiles_x)
{
    switch (method) {
    case WARP_NEAREST: hipLaunchKernelGGL((k21_warp<T, To, WARP_NEAREST>), dim3(grid), dim3(WARP_THREADS), 0, ctx->stream, a, tiles, tiles_x); break;
    case WARP_BILINEAR: hipLaunchKernelGGL((k21_warp<T, To, WARP_BILINEAR>), dim3(grid), dim3(WARP_THREADS), 0, ctx->stream, a, tiles, tiles_x); break;
    case WARP_CUBIC: hipLaunchKernelGGL((k21_warp<T, To, WARP_CUBIC>), dim3(grid), dim3(WARP_THREADS), 0, ctx->stream, a, tiles, tiles_x); break;
    }
}

// the output is the input's dtype, float32 or float64
template <typename T>
void warp_launch_in(rsseg_ctx *ctx, int in_dtype, int out_dtype, int method, const warp_args &a, unsigned grid, int64_t tiles, int tiles_x)
{
    if (out_dtype == in_dtype) warp_launch<T, T>(ctx, method, a, grid, tiles, tiles_x);
    else if (out_dtype == RSSEG_F32) warp_launch<T, float>(ctx, method, a, grid, tiles, tiles_x);
    else warp_launch<T, double>(ctx, method, a, grid, tiles, tiles_x);
}

}  // namespace

extern "C" int rsseg_warp_poly(rsseg_ctx *ctx, const void *const *d_in, int in_dtype, int n_planes, int H, int W, const double *coef, double cx,
                               double cy, int method, double fill, void *const *d_out, int out_dtype, int Ho, int Wo, uint8_t *d_mask,
                               int64_t *n_valid)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    const size_t isz = warp_size(in_dtype), osz = warp_size(out_dtype);
    if (!isz)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: in_dtype %s (%d) not supported: uint8, int16, uint16, int32, float32 or float64",
                       warp_dtype_name(in_dtype), in_dtype);
    if (!osz || (out_dtype != in_dtype && out_dtype != RSSEG_F32 && out_dtype != RSSEG_F64))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: out_dtype %s (%d) not supported for %s planes: the input's dtype, float32 or float64",
                       warp_dtype_name(out_dtype), out_dtype, warp_dtype_name(in_dtype));
    if (ctx->comm_on)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "warp: the source planes must be whole on one GPU (this context has a communication path, "
                                                   "%d ranks): an output pixel may sample any source row", ctx->world);
    if (n_planes < 1 || n_planes > WARP_MAX_BANDS)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: n_planes = %d is not in 1 ... %d", n_planes, WARP_MAX_BANDS);
    if (method != WARP_NEAREST && method != WARP_BILINEAR && method != WARP_CUBIC)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: method = %d is not 0 (nearest), 1 (bilinear) or 2 (cubic)", method);
    if (H < 1 || W < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: H = %d, W = %d: both must be at least 1", H, W);
    if (Ho < 1 || Wo < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: Ho = %d, Wo = %d: both must be at least 1", Ho, Wo);
    const int64_t lim = (int64_t)1 << 39;
    if ((int64_t)H * W >= lim || (int64_t)Ho * Wo >= lim)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "warp: H * W = %lld, Ho * Wo = %lld: both must be below 2^39", (long long)((int64_t)H * W),
                       (long long)((int64_t)Ho * Wo));
    if (!d_in || !d_out || !coef) return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: d_in, d_out or coef is null");
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(coef[i])) return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: coef[%d] = %g is not finite", i, coef[i]);
    if (!std::isfinite(cx) || !std::isfinite(cy)) return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: cx = %g, cy = %g: both must be finite", cx, cy);
    double flo, fhi;
    if (warp_int_range(out_dtype, &flo, &fhi) && !(fill >= flo && fill <= fhi && fill == std::floor(fill)))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: fill = %g is not a value of %s (an integer in %.0f ... %.0f)", fill, warp_dtype_name(out_dtype),
                       flo, fhi);
    warp_args a;
    memset(&a, 0, sizeof(a));
    for (int b = 0; b < n_planes; b++) {
        if (!d_in[b] || !d_out[b] || ((uintptr_t)d_in[b] % isz) || ((uintptr_t)d_out[b] % osz))
            return rs_fail(ctx, RSSEG_ERR_INVALID, "warp: plane %d: d_in and d_out must be non-null and aligned to their element", b);
        a.in[b] = d_in[b];
        a.out[b] = d_out[b];
    }
    for (int i = 0; i < 6; i++) {
        a.p[i] = coef[i];
        a.q[i] = coef[6 + i];
    }
    a.cx = cx;
    a.cy = cy;
    a.fill = fill;
    a.H = H;
    a.W = W;
    a.Ho = Ho;
    a.Wo = Wo;
    a.nb = n_planes;
    a.mask = d_mask;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    RSCHK(ws_reserve(ctx, 64));
    RSCHK(pin_reserve(ctx, 64));
    a.count = (unsigned long long *)ctx->d_ws;
    HIPCHK(ctx, hipMemsetAsync(a.count, 0, sizeof(unsigned long long), ctx->stream));
    // tiles of 4 rows by 64 threads of px pixels each
    const int tiles_x = (int)ceil_div64(Wo, 64 * warp_px(osz, method));
    const int64_t tiles = ceil_div64(Ho, WARP_ROWS) * tiles_x;
    const unsigned grid = (unsigned)std::min<int64_t>(WARP_WG_TARGET, tiles);
    {
        prof_scope ps(ctx, "warp");
        switch (in_dtype) {
        case RSSEG_U8: warp_launch_in<uint8_t>(ctx, in_dtype, out_dtype, method, a, grid, tiles, tiles_x); break;
        case RSSEG_I16: warp_launch_in<int16_t>(ctx, in_dtype, out_dtype, method, a, grid, tiles, tiles_x); break;
        case RSSEG_U16: warp_launch_in<uint16_t>(ctx, in_dtype, out_dtype, method, a, grid, tiles, tiles_x); break;
        case RSSEG_I32: warp_launch_in<int32_t>(ctx, in_dtype, out_dtype, method, a, grid, tiles, tiles_x); break;
        case RSSEG_F32: warp_launch_in<float>(ctx, in_dtype, out_dtype, method, a, grid, tiles, tiles_x); break;
        case RSSEG_F64: warp_launch_in<double>(ctx, in_dtype, out_dtype, method, a, grid, tiles, tiles_x); break;
        }
    }
    HIPCHK(ctx, hipGetLastError());
    if (!n_valid) return stream_sync(ctx);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, a.count, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, rs_sync(ctx));
    *n_valid = (int64_t)((const unsigned long long *)ctx->h_pin)[0];
    return RSSEG_OK;
}
