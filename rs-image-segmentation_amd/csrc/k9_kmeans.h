// Shared by the k-means translation units (k9_kmeans.hip: fit; k18_kmeans_apply.hip: the sweep of a fitted model): the chunk /
// tile / PXL geometry, the plane and scaler arguments, the per-pixel steps both sides must perform with the same operations
// (load_pxf, scaled, tfma), the four-wave sum, the limb arithmetic of the exact sums, and the launch table.
#pragma once
#include <chrono>
#include <type_traits>

#include "common.h"

typedef unsigned __int128 u128;
typedef __int128 i128;

#define KM_THREADS 256
#define KM_TILES_PER_CHUNK 16

template <typename T> struct vt;
template <> struct vt<float> {
    typedef float4 vec;
    static constexpr int PXL = 4;
};
template <> struct vt<double> {
    typedef double2 vec;
    static constexpr int PXL = 2;
};
template <typename T> __host__ __device__ constexpr int km_tile() { return KM_THREADS * vt<T>::PXL; }
template <typename T> __host__ __device__ constexpr int km_chunk() { return km_tile<T>() * KM_TILES_PER_CHUNK; }

struct planes_t {
    const void *p[RSSEG_MAX_FEATURES];
};

// per-feature scaler parameters, in T, resident in device memory (uniform loads)
template <typename T> struct scaler_t {
    T scale[RSSEG_MAX_FEATURES];
    T minv[RSSEG_MAX_FEATURES];
    T mean[RSSEG_MAX_FEATURES];
};

template <typename T> __device__ __forceinline__ T tfma(T a, T b, T c);
template <> __device__ __forceinline__ float tfma<float>(float a, float b, float c) { return __fmaf_rn(a, b, c); }
template <> __device__ __forceinline__ double tfma<double>(double a, double b, double c) { return fma(a, b, c); }

template <typename T> __device__ __forceinline__ void unpack(const typename vt<T>::vec &v, T *o);
template <> __device__ __forceinline__ void unpack<float>(const float4 &v, float *o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
template <> __device__ __forceinline__ void unpack<double>(const double2 &v, double *o) { o[0] = v.x; o[1] = v.y; }

// loads PXL consecutive pixels of plane f starting at pixel `base` (bounds-checked against n)
template <typename T>
__device__ __forceinline__ void load_px(const void *plane, int64_t base, int64_t n, T *o)
{
    constexpr int PXL = vt<T>::PXL;
    const T *p = reinterpret_cast<const T *>(plane);
    if (base + PXL <= n) {
        typename vt<T>::vec v = *reinterpret_cast<const typename vt<T>::vec *>(p + base);
        unpack<T>(v, o);
    } else {
#pragma unroll
        for (int i = 0; i < PXL; i++) o[i] = (base + i < n) ? p[base + i] : (T)0;
    }
}

// FULL: the whole tile lies inside the plane, so the 16-byte load needs no bounds handling
template <typename T, bool FULL>
__device__ __forceinline__ void load_pxf(const void *plane, int64_t base, int64_t n, T *o)
{
    if constexpr (FULL) {
        const T *p = reinterpret_cast<const T *>(plane);
        typedef T ntvec __attribute__((ext_vector_type(vt<T>::PXL)));
        // non-temporal: a sweep streams 16 GB of planes once; nothing is read again before it would be evicted (measured on one
        // box against plain loads: km_moment 2.83 -> 2.65 ms, --data hard 173.1 -> 171.1 ms per step)
        const ntvec v = __builtin_nontemporal_load(reinterpret_cast<const ntvec *>(p + base));
#pragma unroll
        for (int i = 0; i < vt<T>::PXL; i++) o[i] = v[i];
    } else {
        if (base < n) load_px<T>(plane, base, n, o);
        else {
#pragma unroll
            for (int i = 0; i < vt<T>::PXL; i++) o[i] = (T)0;
        }
    }
}

// Plane f of a FULL tile for the software-pipelined walks (k9_kmeans.hip): always exactly one 16-byte request, on every path.
// A plane beyond F repeats plane F - 1 — a line the lane has just asked for, never an address outside a plane — and its
// value is not used.  With `if (f < F)` around a load the compiler cannot count the requests between a load and its first use
// (the count differs between the paths that meet behind the branch) and waits for ALL outstanding loads, the next tile's
// included; with a fixed count it waits for the one plane it needs and leaves the later ones in flight.
// The address is (plane + chunk0), uniform, plus the lane's 32-bit pixel offset inside the chunk: one offset register serves
// all planes (scalar base + vector offset addressing) instead of a 64-bit address pair per plane.
template <typename T>
__device__ __forceinline__ void load_pxq(const planes_t &pl, int F, int f, int64_t chunk0, uint32_t off, T *o)
{
    typedef T ntvec __attribute__((ext_vector_type(vt<T>::PXL)));
    const char *p = reinterpret_cast<const char *>(reinterpret_cast<const T *>(pl.p[f < F ? f : F - 1]) + chunk0);
    const ntvec v = __builtin_nontemporal_load(reinterpret_cast<const ntvec *>(p + (size_t)(off * (uint32_t)sizeof(T))));
#pragma unroll
    for (int i = 0; i < vt<T>::PXL; i++) o[i] = v[i];
}

template <typename T> __device__ __forceinline__ T scaled(T x, T sc, T mn)
{
    if (x != x) x = (T)0;  // extract.py:548-556  NaN -> 0
    T xs = x * sc;
    return xs + mn;
}

// The four-wave sum of this file's kernels, in two halves around the caller's one __syncthreads(): wg_put leaves a wave's sum
// (wave_sum) in s[wave] — lane 0 writes, both values in one go where a kernel reduces two — and wg_sum adds the four.
template <typename V> __device__ __forceinline__ void wg_put(V *s, V v)
{
    if (lane_id() == 0) s[threadIdx.x >> 6] = v;
}
template <typename V> __device__ __forceinline__ void wg_put(V *s0, V v0, V *s1, V v1)
{
    if (lane_id() == 0) { s0[threadIdx.x >> 6] = v0; s1[threadIdx.x >> 6] = v1; }
}
template <typename V> __device__ __forceinline__ V wg_sum(const V *s) { return s[0] + s[1] + s[2] + s[3]; }

// the feature-blocked kernels (33 ... 64 planes) walk a tile's planes in blocks of KM_FB
#define KM_FB 16

template <typename T, bool FULL>
__device__ __forceinline__ void load_block(const planes_t &pl, int F, int f0, int64_t base, int64_t n, T (&x)[KM_FB][vt<T>::PXL])
{
#pragma unroll
    for (int j = 0; j < KM_FB; j++) {
        if (f0 + j < F) load_pxf<T, FULL>(pl.p[f0 + j], base, n, x[j]);
        else {
#pragma unroll
            for (int p = 0; p < vt<T>::PXL; p++) x[j][p] = (T)0;
        }
    }
}

// combine {hi, lo} limb sums (km_reduce_cols) into one signed 128-bit value
__host__ __device__ __forceinline__ i128 limbs(long long hi, long long lo) { return ((i128)hi << 32) + (i128)lo; }
template <typename T> __host__ __device__ __forceinline__ T fixed_to_T(i128 s) { return (T)((double)s * (1.0 / 1099511627776.0)); }

// column sums of partial[rows][nchunks] -> out[rows][2] = {sum of (v >> 32), sum of (v & 0xffffffff)} on ctx's stream
// (km_reduce_cols, k9_kmeans.hip)
__attribute__((visibility("hidden"))) int km_reduce_cols_launch(rsseg_ctx *ctx, const long long *partial, int64_t nchunks, int rows, long long *out);

namespace {

inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the launch table: which instantiation serves (T, KMAX, F) ----
// A kernel holds FR = 8, 16 or 32 planes of its pixels in registers, or KM_BLOCKED for 33 ... RSSEG_MAX_FEATURES planes:
// km_kpp_blk / km_lloyd_blk then hold one block of KM_FB planes at a time, km_farthest<T, KMAX, 64> all of them.
constexpr int KM_BLOCKED = 64;
static_assert(RSSEG_MAX_FEATURES <= KM_BLOCKED, "km_farthest<T, KMAX, KM_BLOCKED> holds every plane");
constexpr int km_width(int F) { return F <= 8 ? 8 : (F <= 16 ? 16 : (F <= 32 ? 32 : KM_BLOCKED)); }
constexpr int km_kmax(int k) { return k <= 8 ? 8 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64)); }

// The Lloyd kernel of (T, KMAX, F).  float64 planes with 33 ... 64 clusters: the register-resident kernels for 9 ... 32 planes
// would need more than 512 registers (252 - 628 bytes of scratch per lane in the r03 code object), so they take
// the feature-blocked kernel, which holds one block of planes at a time (346 - 370 registers), same arithmetic, same bits.
template <typename T> constexpr int lloyd_form(int KMAX, int F)
{
    return std::is_same<T, double>::value && KMAX == 64 && F > 8 ? KM_BLOCKED : km_width(F);
}
// Only the register-resident kernels write the caller's int32 plane themselves (km_lloyd's out32, final E-step).
template <typename T> constexpr bool lloyd_writes_int32(int KMAX, int F) { return lloyd_form<T>(KMAX, F) != KM_BLOCKED; }

// runtime value -> template argument: fn(std::integral_constant<int, V>) for V = KMAX (8, 16, 32, 64) or a width (8, 16, 32, KM_BLOCKED)
template <int V> using ic = std::integral_constant<int, V>;
template <typename Fn> auto with_kmax(int KMAX, Fn &&fn)
{
    switch (KMAX) {
    case 8: return fn(ic<8>());
    case 16: return fn(ic<16>());
    case 32: return fn(ic<32>());
    default: return fn(ic<64>());
    }
}
template <typename Fn> auto with_width(int FR, Fn &&fn)
{
    switch (FR) {
    case 8: return fn(ic<8>());
    case 16: return fn(ic<16>());
    case 32: return fn(ic<32>());
    default: return fn(ic<KM_BLOCKED>());
    }
}

}  // namespace
