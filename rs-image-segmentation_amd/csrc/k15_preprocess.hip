// K15 — stage 1 of the reference: radiometric calibration, the identity warp and the 8-bit min-max stretch of
// modules/features/preprocessing.py:54-125 as scripts/1_preprocessing.py:25-85 chains them, from DN planes of one dtype to
// uint8 planes that stay in HBM for the feature stage.
//
// Per band i, NumPy 2 computes radiance = gain[i] * band + bias[i] in float64 (float32 for float32 DN: the Python floats are
// rounded to float32 first), then ((radiance - mn) * 255.0) / (mx - mn) in that dtype with mn / mx = np.min / np.max of the
// radiance (NaN when the band holds one), then .astype(np.uint8).  Gains are > 0, so radiance is monotone in DN and IEEE
// rounding keeps it monotone: np.min(radiance) == gain * np.min(DN) + bias bit for bit.  Hence two passes:
//   k15_range    per band, min / max of the non-NaN DN and the NaN count (one partial per workgroup; k15_reduce folds them
//                into the reduced record, no initialised device state, no atomics);
//   k15_stretch  per pixel the same IEEE expression as NumPy, after each workgroup derives the radiance range from the
//                reduced record in its prologue.  8-bit DN go through a 256-entry LUT built in LDS by that prologue.
// Both read 16 bytes per lane and instruction, grid-stride; workgroup 0 of each band takes the tail that is not a whole vector.

#include "common.h"

#include <climits>
#include <cmath>

#define PRE_THREADS 256
#define PRE_UNROLL 4
#define PRE_WG_TARGET 2048   // workgroups per pass over all bands: 8 of 256 threads per CU
#define PRE_MAX_BANDS 16

struct pre_args {
    const void *in[PRE_MAX_BANDS];
    uint8_t *out[PRE_MAX_BANDS];
    double gain[PRE_MAX_BANDS], bias[PRE_MAX_BANDS];
    int64_t n;   // pixels per band (this rank's)
    int nb;      // bands
};

// the dtype of the radiance NumPy computes: float32 for float32 DN, float64 otherwise
template <typename T> struct pre_real { typedef double R; };
template <> struct pre_real<float> { typedef float R; };
// what the range pass accumulates in: the DN's own ordering, NaN-ignoring for the float types
template <typename T> struct pre_acc { typedef int A; };
template <> struct pre_acc<int32_t> { typedef int32_t A; };
template <> struct pre_acc<float> { typedef float A; };
template <> struct pre_acc<double> { typedef double A; };

template <typename T>
__device__ __forceinline__ void pre_unpack(const rs_u4v &u, T (&x)[16 / sizeof(T)])
{
    union {
        rs_u4v u;
        T t[16 / sizeof(T)];
    } b;
    b.u = u;
#pragma unroll
    for (int e = 0; e < (int)(16 / sizeof(T)); e++) x[e] = b.t[e];
}

template <typename A> __device__ __forceinline__ A pre_min(A a, A b) { return b < a ? b : a; }
template <typename A> __device__ __forceinline__ A pre_max(A a, A b) { return b > a ? b : a; }
// fmin / fmax drop a NaN operand: the NaN-ignoring extrema the NaN count is kept beside
template <> __device__ __forceinline__ float pre_min(float a, float b) { return fminf(a, b); }
template <> __device__ __forceinline__ float pre_max(float a, float b) { return fmaxf(a, b); }
template <> __device__ __forceinline__ double pre_min(double a, double b) { return fmin(a, b); }
template <> __device__ __forceinline__ double pre_max(double a, double b) { return fmax(a, b); }
template <typename A> __device__ __forceinline__ A pre_lowest() { return std::is_floating_point<A>::value ? (A)-INFINITY : std::numeric_limits<A>::lowest(); }
template <typename A> __device__ __forceinline__ A pre_highest() { return std::is_floating_point<A>::value ? (A)INFINITY : std::numeric_limits<A>::max(); }

// part = {min[nb][G], max[nb][G]} as double (exact for every DN dtype), then nan[nb][G] as int64.  A workgroup without a
// non-NaN value writes (+inf, -inf).
template <typename T>
__global__ __launch_bounds__(PRE_THREADS) void k15_range(const pre_args a, double *__restrict__ part)
{
    typedef typename pre_acc<T>::A A;
    constexpr int P = 16 / sizeof(T);
    constexpr bool FP = std::is_floating_point<T>::value;
    const int b = blockIdx.y, G = gridDim.x;
    const T *x = (const T *)a.in[b];
    const rs_u4v *src = (const rs_u4v *)x;
    A mn = pre_highest<A>(), mx = pre_lowest<A>();
    long long nan = 0;
    auto take = [&](T v) {
        mn = pre_min<A>(mn, (A)v);
        mx = pre_max<A>(mx, (A)v);
        if (FP) nan += v != v;
    };
    const int64_t nv = a.n / P, stride = (int64_t)G * PRE_THREADS;
    int64_t v = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x;
    for (; v + (PRE_UNROLL - 1) * stride < nv; v += PRE_UNROLL * stride) {
        rs_u4v u[PRE_UNROLL];
#pragma unroll
        for (int k = 0; k < PRE_UNROLL; k++) u[k] = __builtin_nontemporal_load(src + v + k * stride);
#pragma unroll
        for (int k = 0; k < PRE_UNROLL; k++) {
            T t[P];
            pre_unpack<T>(u[k], t);
#pragma unroll
            for (int e = 0; e < P; e++) take(t[e]);
        }
    }
    for (; v < nv; v += stride) {
        T t[P];
        pre_unpack<T>(__builtin_nontemporal_load(src + v), t);
#pragma unroll
        for (int e = 0; e < P; e++) take(t[e]);
    }
    if (blockIdx.x == 0)
        for (int64_t i = nv * P + threadIdx.x; i < a.n; i += PRE_THREADS) take(x[i]);
    double dmn = (double)mn, dmx = (double)mx;
    if (!FP) {   // the integer sentinels of an empty workgroup become the float ones
        if (mn == pre_highest<A>() && mx == pre_lowest<A>() && mx < mn) { dmn = INFINITY; dmx = -INFINITY; }
    }
    dmn = wave_min(dmn);
    dmx = wave_max(dmx);
    nan = wave_sum(nan);
    __shared__ double s_mn[PRE_THREADS / 64], s_mx[PRE_THREADS / 64];
    __shared__ long long s_nan[PRE_THREADS / 64];
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { s_mn[w] = dmn; s_mx[w] = dmx; s_nan[w] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < PRE_THREADS / 64; i++) { dmn = fmin(dmn, s_mn[i]); dmx = fmax(dmx, s_mx[i]); nan += s_nan[i]; }
        const size_t o = (size_t)b * G + blockIdx.x;
        part[o] = dmn;
        part[(size_t)a.nb * G + o] = dmx;
        reinterpret_cast<long long *>(part)[(size_t)2 * a.nb * G + o] = nan;
    }
}

// one workgroup per band: red = {min[nb], max[nb]} (double), then nan[nb] (int64) — the record the hook reduces
__global__ __launch_bounds__(PRE_THREADS) void k15_reduce(const double *__restrict__ part, int G, int nb, char *__restrict__ red)
{
    const int b = blockIdx.x;
    double mn = INFINITY, mx = -INFINITY;
    long long nan = 0;
    const long long *pn = reinterpret_cast<const long long *>(part) + (size_t)2 * nb * G;
    for (int i = threadIdx.x; i < G; i += PRE_THREADS) {
        mn = fmin(mn, part[(size_t)b * G + i]);
        mx = fmax(mx, part[(size_t)nb * G + (size_t)b * G + i]);
        nan += pn[(size_t)b * G + i];
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    nan = wave_sum(nan);
    __shared__ double s_mn[PRE_THREADS / 64], s_mx[PRE_THREADS / 64];
    __shared__ long long s_nan[PRE_THREADS / 64];
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) { s_mn[w] = mn; s_mx[w] = mx; s_nan[w] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < PRE_THREADS / 64; i++) { mn = fmin(mn, s_mn[i]); mx = fmax(mx, s_mx[i]); nan += s_nan[i]; }
        double *r = reinterpret_cast<double *>(red);
        r[b] = mn;
        r[nb + b] = mx;
        reinterpret_cast<long long *>(red)[2 * nb + b] = nan;
    }
}

// the stretch of one value, given the radiance range: ((radiance - lo) * 255) / (hi - lo) in R, then astype(uint8) as x86-64
// NumPy casts (truncation on [0, 256), 0 for NaN and +-inf; the expression cannot give another finite value)
template <typename T, bool CAL>
struct pre_map {
    typedef typename pre_real<T>::R R;
    R g, c, lo, den;
    __device__ __forceinline__ pre_map(const pre_args &a, const char *red, int b)
    {
        const double *r = reinterpret_cast<const double *>(red);
        g = (R)a.gain[b];
        c = (R)a.bias[b];
        R mn = (R)r[b], mx = (R)r[a.nb + b];   // exact: the DN extrema are values of T
        if (CAL) {   // gain > 0 and monotone rounding: the radiance extrema are those of the DN, calibrated
            mn = g * mn + c;
            mx = g * mx + c;
        }
        if (reinterpret_cast<const long long *>(red)[2 * a.nb + b] > 0) mn = mx = (R)NAN;   // np.min / np.max propagate NaN
        lo = mn;
        den = mx - mn;
    }
    __device__ __forceinline__ uint8_t operator()(T x) const
    {
        R r = (R)x;
        if (CAL) r = g * r + c;
        const R v = ((r - lo) * (R)255) / den;
        return v >= (R)0 && v < (R)256 ? (uint8_t)(unsigned)v : (uint8_t)0;
    }
};

template <int P> struct pre_bytes;
template <> struct pre_bytes<2> { typedef uint16_t U; };
template <> struct pre_bytes<4> { typedef uint32_t U; };
template <> struct pre_bytes<8> { typedef uint64_t U; };

// direct evaluation (16-, 32- and 64-bit DN): P uint8 results per 16-byte vector, stored as one P-byte word
template <typename T, bool CAL>
__global__ __launch_bounds__(PRE_THREADS) void k15_stretch(const pre_args a, const char *__restrict__ red)
{
    constexpr int P = 16 / sizeof(T);
    typedef typename pre_bytes<P>::U U;
    const int b = blockIdx.y;
    const pre_map<T, CAL> f(a, red, b);
    const T *x = (const T *)a.in[b];
    const rs_u4v *src = (const rs_u4v *)x;
    uint8_t *out = a.out[b];
    U *dst = (U *)out;
    auto one = [&](const rs_u4v &u, int64_t v) {
        T t[P];
        pre_unpack<T>(u, t);
        union {
            U w;
            uint8_t q[P];
        } o;
#pragma unroll
        for (int e = 0; e < P; e++) o.q[e] = f(t[e]);
        dst[v] = o.w;
    };
    const int64_t nv = a.n / P, stride = (int64_t)gridDim.x * PRE_THREADS;
    int64_t v = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x;
    for (; v + (PRE_UNROLL - 1) * stride < nv; v += PRE_UNROLL * stride) {
        rs_u4v u[PRE_UNROLL];
#pragma unroll
        for (int k = 0; k < PRE_UNROLL; k++) u[k] = __builtin_nontemporal_load(src + v + k * stride);
#pragma unroll
        for (int k = 0; k < PRE_UNROLL; k++) one(u[k], v + k * stride);
    }
    for (; v < nv; v += stride) one(__builtin_nontemporal_load(src + v), v);
    if (blockIdx.x == 0)
        for (int64_t i = nv * P + threadIdx.x; i < a.n; i += PRE_THREADS) out[i] = f(x[i]);
}

// 8-bit DN: the prologue evaluates the 256 possible values into an LDS table, the body is a byte gather
template <bool CAL>
__global__ __launch_bounds__(PRE_THREADS) void k15_stretch_u8(const pre_args a, const char *__restrict__ red)
{
    static_assert(PRE_THREADS == 256, "one LUT entry per thread");
    __shared__ uint8_t lut[256];
    const int b = blockIdx.y;
    {
        const pre_map<uint8_t, CAL> f(a, red, b);
        lut[threadIdx.x] = f((uint8_t)threadIdx.x);
    }
    __syncthreads();
    const uint8_t *x = (const uint8_t *)a.in[b];
    const rs_u4v *src = (const rs_u4v *)x;
    uint8_t *out = a.out[b];
    rs_u4v *dst = (rs_u4v *)out;
    auto one = [&](const rs_u4v &u, int64_t v) {
        union {
            rs_u4v u;
            uint8_t q[16];
        } s, o;
        s.u = u;
#pragma unroll
        for (int e = 0; e < 16; e++) o.q[e] = lut[s.q[e]];
        dst[v] = o.u;
    };
    const int64_t nv = a.n / 16, stride = (int64_t)gridDim.x * PRE_THREADS;
    int64_t v = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x;
    for (; v + (PRE_UNROLL - 1) * stride < nv; v += PRE_UNROLL * stride) {
        rs_u4v u[PRE_UNROLL];
#pragma unroll
        for (int k = 0; k < PRE_UNROLL; k++) u[k] = __builtin_nontemporal_load(src + v + k * stride);
#pragma unroll
        for (int k = 0; k < PRE_UNROLL; k++) one(u[k], v + k * stride);
    }
    for (; v < nv; v += stride) one(__builtin_nontemporal_load(src + v), v);
    if (blockIdx.x == 0)
        for (int64_t i = nv * 16 + threadIdx.x; i < a.n; i += PRE_THREADS) out[i] = lut[x[i]];
}

// rsseg_radiometric: gain * x + bias in R, elementwise
template <typename T>
__global__ __launch_bounds__(PRE_THREADS) void k15_radiometric(const T *__restrict__ x, int64_t n, double gain, double bias,
                                                               typename pre_real<T>::R *__restrict__ out)
{
    typedef typename pre_real<T>::R R;
    const R g = (R)gain, c = (R)bias;
    const int64_t stride = (int64_t)gridDim.x * PRE_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * PRE_THREADS + threadIdx.x; i < n; i += stride) out[i] = g * (R)x[i] + c;
}

namespace {

const char *pre_dtype_name(int dtype)
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

size_t pre_size(int dtype)
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

template <typename T>
int pre_launch(rsseg_ctx *ctx, const pre_args &a, int G, double *d_part, char *d_red, bool cal, bool stretch)
{
    if (!stretch) {
        prof_scope ps(ctx, "pre_range");
        hipLaunchKernelGGL(k15_range<T>, dim3(G, a.nb), dim3(PRE_THREADS), 0, ctx->stream, a, d_part);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k15_reduce, dim3(a.nb), dim3(PRE_THREADS), 0, ctx->stream, (const double *)d_part, G, a.nb, d_red);
        HIPCHK(ctx, hipGetLastError());
        return RSSEG_OK;
    }
    prof_scope ps(ctx, "pre_stretch");
    if constexpr (sizeof(T) == 1) {
        if (cal) hipLaunchKernelGGL(k15_stretch_u8<true>, dim3(G, a.nb), dim3(PRE_THREADS), 0, ctx->stream, a, (const char *)d_red);
        else hipLaunchKernelGGL(k15_stretch_u8<false>, dim3(G, a.nb), dim3(PRE_THREADS), 0, ctx->stream, a, (const char *)d_red);
    } else {
        if (cal) hipLaunchKernelGGL((k15_stretch<T, true>), dim3(G, a.nb), dim3(PRE_THREADS), 0, ctx->stream, a, (const char *)d_red);
        else hipLaunchKernelGGL((k15_stretch<T, false>), dim3(G, a.nb), dim3(PRE_THREADS), 0, ctx->stream, a, (const char *)d_red);
    }
    HIPCHK(ctx, hipGetLastError());
    return RSSEG_OK;
}

int pre_dispatch(rsseg_ctx *ctx, int dtype, const pre_args &a, int G, double *d_part, char *d_red, bool cal, bool stretch)
{
    switch (dtype) {
    case RSSEG_U8: return pre_launch<uint8_t>(ctx, a, G, d_part, d_red, cal, stretch);
    case RSSEG_I16: return pre_launch<int16_t>(ctx, a, G, d_part, d_red, cal, stretch);
    case RSSEG_U16: return pre_launch<uint16_t>(ctx, a, G, d_part, d_red, cal, stretch);
    case RSSEG_I32: return pre_launch<int32_t>(ctx, a, G, d_part, d_red, cal, stretch);
    case RSSEG_F32: return pre_launch<float>(ctx, a, G, d_part, d_red, cal, stretch);
    case RSSEG_F64: return pre_launch<double>(ctx, a, G, d_part, d_red, cal, stretch);
    }
    return RSSEG_ERR_INVALID;
}

}  // namespace

extern "C" int rsseg_preprocess_u8(rsseg_ctx *ctx, const void *const *d_in, int in_dtype, int n_bands, int64_t n_local, const double *gain,
                                   const double *bias, uint8_t *const *d_out, double *range_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    const size_t esz = pre_size(in_dtype);
    if (!esz)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "preprocess: input dtype %s (%d) not supported: uint8, int16, uint16, int32, float32 or float64",
                       pre_dtype_name(in_dtype), in_dtype);
    if (n_bands < 1 || n_bands > PRE_MAX_BANDS || n_local < 0 || !d_in || !d_out || (!gain) != (!bias))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "preprocess: bad arguments (bands=%d n=%lld, gain and bias both given or both NULL)", n_bands,
                       (long long)n_local);
    pre_args a;
    memset(&a, 0, sizeof(a));
    a.n = n_local;
    a.nb = n_bands;
    for (int b = 0; b < n_bands; b++) {
        if (gain) {
            if (!std::isfinite(gain[b]) || !std::isfinite(bias[b]) || !(gain[b] > 0.0))
                return rs_fail(ctx, RSSEG_ERR_INVALID, "preprocess: band %d gain %g, bias %g: the gain must be finite and > 0, the bias finite", b,
                               gain[b], bias[b]);
            a.gain[b] = gain[b];
            a.bias[b] = bias[b];
        }
        if (n_local > 0 && (!d_in[b] || !d_out[b] || ((uintptr_t)d_in[b] & 15) || ((uintptr_t)d_out[b] & 15)))
            return rs_fail(ctx, RSSEG_ERR_INVALID, "preprocess: band %d: planes must be non-null and 16-byte aligned", b);
        a.in[b] = d_in[b];
        a.out[b] = d_out[b];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int64_t nv = n_local / (int64_t)(16 / esz);
    const int G = (int)std::min<int64_t>(std::max(1, PRE_WG_TARGET / n_bands), std::max<int64_t>(1, ceil_div64(nv, (int64_t)PRE_THREADS * PRE_UNROLL)));
    const size_t part_bytes = (size_t)3 * 8 * n_bands * G, red_bytes = (size_t)3 * 8 * n_bands;
    if (ctx->comm_on && red_bytes > ctx->comm_bytes)
        return rs_fail(ctx, RSSEG_ERR_COMM, "preprocess: comm buffer too small (%zu > %zu)", red_bytes, ctx->comm_bytes);
    RSCHK(ws_reserve(ctx, part_bytes + red_bytes));
    double *d_part = (double *)ctx->d_ws;
    // the reduced record lives where the hook reduces it: the communication buffer when a hook is installed
    char *d_red = ctx->comm_on ? ctx->d_comm : ctx->d_ws + part_bytes;
    const bool cal = gain != nullptr;

    RSCHK(pre_dispatch(ctx, in_dtype, a, G, d_part, d_red, cal, false));
    RSCHK(comm_allreduce_dev(ctx, 0, n_bands, RSSEG_F64, RSSEG_MIN));
    RSCHK(comm_allreduce_dev(ctx, 8 * (int64_t)n_bands, n_bands, RSSEG_F64, RSSEG_MAX));
    RSCHK(comm_allreduce_dev(ctx, 16 * (int64_t)n_bands, n_bands, RSSEG_I64, RSSEG_SUM));
    if (n_local > 0) RSCHK(pre_dispatch(ctx, in_dtype, a, G, d_part, d_red, cal, true));
    if (range_out) {   // the one host wait: the whole raster's DN range per band
        RSCHK(pin_reserve(ctx, red_bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_red, red_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, rs_sync(ctx));
        const double *h = (const double *)ctx->h_pin;
        const long long *hn = (const long long *)ctx->h_pin + 2 * n_bands;
        for (int b = 0; b < n_bands; b++) {
            range_out[3 * b] = h[b];
            range_out[3 * b + 1] = h[n_bands + b];
            range_out[3 * b + 2] = (double)hn[b];
        }
    }
    return RSSEG_OK;
}

extern "C" int rsseg_radiometric(rsseg_ctx *ctx, const void *d_in, int in_dtype, int64_t n, double gain, double bias, void *d_out)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!pre_size(in_dtype))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "radiometric: input dtype %s (%d) not supported: uint8, int16, uint16, int32, float32 or float64",
                       pre_dtype_name(in_dtype), in_dtype);
    if (n < 0 || (n > 0 && (!d_in || !d_out)) || !std::isfinite(gain) || !std::isfinite(bias))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "radiometric: bad arguments (n=%lld gain %g bias %g)", (long long)n, gain, bias);
    if (n == 0) return RSSEG_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int grid = (int)std::min<int64_t>(4096, ceil_div64(n, PRE_THREADS));
#define PRE_RAD(T)                                                                                                               \
    hipLaunchKernelGGL(k15_radiometric<T>, dim3(grid), dim3(PRE_THREADS), 0, ctx->stream, (const T *)d_in, n, gain, bias,     \
                       (typename pre_real<T>::R *)d_out);                                                                     \
    break
    switch (in_dtype) {
    case RSSEG_U8: PRE_RAD(uint8_t);
    case RSSEG_I16: PRE_RAD(int16_t);
    case RSSEG_U16: PRE_RAD(uint16_t);
    case RSSEG_I32: PRE_RAD(int32_t);
    case RSSEG_F32: PRE_RAD(float);
    case RSSEG_F64: PRE_RAD(double);
    }
#undef PRE_RAD
    HIPCHK(ctx, hipGetLastError());
    return stream_sync(ctx);
}
