// K18 — rsseg_kmeans_predict: a fitted KMeans model (MinMaxScaler + cluster centres) applied to feature-planar rasters.
// The per-pixel steps it shares with the fit (k9_kmeans.hip) come from k9_kmeans.h.
#include <algorithm>
#include <cmath>

#include "k9_kmeans.h"

// ------------------------------------------------------------------------------------------------
// K18 — the assignment sweep of a FITTED model (rsseg_kmeans_predict): MinMaxScaler.transform + KMeans.predict, and on
// request the distance of every pixel to its centre and the per-cluster counts / inertia of the scene.
//   sklearn/cluster/_kmeans.py:1060-1110 (predict, score -> _labels_inertia)   _k_means_common.pyx:16-43,102-135
// Per pixel, in T, the E-step of km_lloyd on UNCENTRED values (cluster_centers_ has the fit's mean added back):
//   xs_f = scaled(x_f); dot_j = fma chain over f; d_j = fma(-2, dot_j, csq_j); label = lowest j with the strictly smallest d_j;
//   sq = _euclidean_dense_dense(xs, c_label, squared=True): per group of four features ((d0^2 + d1^2) + d2^2) + d3^2 added to
//   the running result, the remaining features one at a time; dist = sqrt(sq), correctly rounded (ka_sqrt).
// MODE (compile time): KA_DIST writes the distance plane, KA_SUM leaves the chunk's counts, inertia and overflow count in
// `partial`; MODE 0 (labels only) holds no centre rows, reads no LDS and does none of the distance arithmetic.
// The centre of a pixel's label is a PER-LANE row.  The rows lie in LDS row-major with a row stride of F | 1 elements: an odd
// stride is a permutation of the banks (ds_read_b32: word mod 32 within a group of 32 lanes; ds_read_b64: element mod 32), so
// lanes whose labels differ modulo 32 read different banks and lanes with the same label read one address (a broadcast).  The
// worst case is 2-way (labels j and j + 32 in one lane group).  Wider reads (four features per ds_read_b128) would need a
// stride of 4 x odd words and a fourth of the instructions; the F * PXL reads of a tile (60 at F = 15: 120 LDS cycles per wave)
// are a tenth of the ~1260 clocks a CU's share of HBM needs for the wave's 16 KB of planes, so the plain form stays.
// The dot products read the transposed centres through uniform loads as km_lloyd does.
// Inertia: the sum of llrint(sq * 2^40), exact.  A lane adds its pixels' quanta in a register, the workgroup's four waves are
// added (wave_sum / wg_put / wg_sum) into ONE signed 64-bit partial per chunk, km_reduce_cols adds the chunks as limbs.  A
// pixel is summed only while its quanta stay below 2^63 / chunk (so that a chunk's partial cannot leave the signed range):
// sq < 2^23 / chunk - 2^-41, i.e. 512 for float32 (chunk 16384) and 1024 for float64 (chunk 8192), both inside the 2^11 the
// magic-number conversion holds (common.h, to_fixed40).  Any other pixel (also a non-finite sq) counts in the overflow row.
// Counts: LDS atomics on KA_COPIES bank-private copies (copy = lane & 31, odd stride), as km_lloyd's.
// The chunk walk, the dot products and the argmin are km_lloyd's / km_lloyd_blk's (k9_kmeans.hip), statement for statement.
// ------------------------------------------------------------------------------------------------
#define KA_DIST 1
#define KA_SUM 2
#define KA_COPIES 32
__host__ __device__ inline int ka_row_stride(int F) { return F | 1; }
template <typename T> __host__ __device__ inline size_t ka_cen_bytes(int mode, int KMAX, int F)
{
    return mode ? (sizeof(T) * (size_t)KMAX * ka_row_stride(F) + 15) & ~(size_t)15 : 0;
}
__host__ __device__ inline int ka_cnt_stride(int KMAX) { return KMAX | 1; }   // in 8-byte words
template <typename T> __host__ __device__ inline size_t ka_lds_bytes(int mode, int KMAX, int F)
{
    return ka_cen_bytes<T>(mode, KMAX, F) + ((mode & KA_SUM) ? sizeof(long long) * (size_t)KA_COPIES * ka_cnt_stride(KMAX) : 0);
}
// quanta (2^-40) a pixel may add to its chunk's partial: below 2^63 / chunk
template <typename T> __host__ __device__ constexpr long long ka_qmax() { return (1LL << 62) / (km_chunk<T>() / 2); }

// The distance's square root, correctly rounded in both types.  (t_sqrt<float> is __fsqrt_rn, which this toolchain maps to the
// native approximation: good for kl_update, whose result is squared again and compared, not for a value that is returned.)
template <typename T> __device__ __forceinline__ T ka_sqrt(T x);
template <> __device__ __forceinline__ float ka_sqrt<float>(float x) { return sqrtf(x); }
template <> __device__ __forceinline__ double ka_sqrt<double>(double x) { return sqrt(x); }

// centre rows into LDS (row-major, stride F | 1) and zeroed counter copies; all threads, ends with the barrier
template <typename T, int MODE>
__device__ __forceinline__ void ka_fill_lds(char *smem, int KMAX, int F, int k, const T *__restrict__ cenT)
{
    if constexpr (MODE != 0) {
        T *cen_s = reinterpret_cast<T *>(smem);
        const int rs = ka_row_stride(F);
        for (int i = threadIdx.x; i < k * F; i += KM_THREADS) {
            const int j = i / F, f = i - j * F;
            cen_s[j * rs + f] = cenT[f * KMAX + j];
        }
        if constexpr ((MODE & KA_SUM) != 0) {
            unsigned long long *S = reinterpret_cast<unsigned long long *>(smem + ka_cen_bytes<T>(MODE, KMAX, F));
            for (int i = threadIdx.x; i < KA_COPIES * ka_cnt_stride(KMAX); i += KM_THREADS) S[i] = 0ull;
        }
        __syncthreads();
    }
}

// labels (and distances) of a lane's PXL pixels: 16-byte stores when the tile is whole and the plane aligned (`vec`)
template <typename T, bool FULL>
__device__ __forceinline__ void ka_store(int32_t *__restrict__ out32, T *__restrict__ dist, bool want_dist, int64_t base, int64_t n, int vec,
                                         const int (&lab)[vt<T>::PXL], const T (&dv)[vt<T>::PXL])
{
    constexpr int PXL = vt<T>::PXL;
    if ((vec & 1) && (FULL || base + PXL <= n)) {
        if constexpr (PXL == 4) *reinterpret_cast<int4 *>(out32 + base) = make_int4(lab[0], lab[1], lab[2], lab[3]);
        else *reinterpret_cast<int2 *>(out32 + base) = make_int2(lab[0], lab[1]);
    } else {
#pragma unroll
        for (int p = 0; p < PXL; p++)
            if (FULL || base + p < n) out32[base + p] = lab[p];
    }
    if (want_dist) {
        if ((vec & 2) && (FULL || base + PXL <= n)) {
            typename vt<T>::vec v;
            if constexpr (PXL == 4) { v.x = dv[0]; v.y = dv[1]; v.z = dv[2]; v.w = dv[3]; }
            else { v.x = dv[0]; v.y = dv[1]; }
            *reinterpret_cast<typename vt<T>::vec *>(dist + base) = v;
        } else {
#pragma unroll
            for (int p = 0; p < PXL; p++)
                if (FULL || base + p < n) dist[base + p] = dv[p];
        }
    }
}

// the summary's share of a lane's PXL pixels: counts into the lane's counter copy, quanta and overflows into its registers
template <typename T, bool FULL>
__device__ __forceinline__ void ka_tally(unsigned long long *myS, int64_t base, int64_t n, const int (&lab)[vt<T>::PXL],
                                         const T (&sq)[vt<T>::PXL], long long &my_q, long long &my_ovf)
{
    constexpr int PXL = vt<T>::PXL;
    bool valid[PXL];
#pragma unroll
    for (int p = 0; p < PXL; p++) valid[p] = FULL || base + p < n;
    bool same = valid[PXL - 1];
#pragma unroll
    for (int p = 1; p < PXL; p++) same = same && lab[p] == lab[0];
    if (same) {
        atomicAdd(&myS[lab[0]], (unsigned long long)PXL);
    } else {
#pragma unroll
        for (int p = 0; p < PXL; p++)
            if (valid[p]) atomicAdd(&myS[lab[p]], 1ull);
    }
#pragma unroll
    for (int p = 0; p < PXL; p++)
        if (valid[p]) {
            long long q = ka_qmax<T>();
            if (sq[p] < (T)2048) q = to_fixed40((double)sq[p]);   // NaN compares false
            if (q < ka_qmax<T>()) my_q += q;
            else my_ovf += 1;
        }
}

// rows of `partial`: [0, KMAX) counts, KMAX the inertia quanta, KMAX + 1 the pixels left out of it
template <typename T>
__device__ __forceinline__ void ka_epilogue(const unsigned long long *S, int KMAX, long long my_q, long long my_ovf,
                                            long long *__restrict__ partial, int64_t nchunks)
{
    __shared__ long long q_w[4], ovf_w[4];
    wg_put(q_w, wave_sum(my_q), ovf_w, wave_sum(my_ovf));
    __syncthreads();
    const int stride = ka_cnt_stride(KMAX);
    for (int i = threadIdx.x; i < KMAX + 2; i += KM_THREADS) {
        long long v;
        if (i < KMAX) {
            unsigned long long a = 0;
            for (int c = 0; c < KA_COPIES; c++) a += S[(size_t)c * stride + i];
            v = (long long)a;
        } else {
            v = i == KMAX ? wg_sum(q_w) : wg_sum(ovf_w);
        }
        partial[(size_t)i * nchunks + blockIdx.x] = v;
    }
}

// register-resident form: FR = 8 / 16 / 32 planes of the lane's pixels stay in registers from the dot products to the distance
template <typename T, int KMAX, int FR, int MODE>
__global__ __launch_bounds__(KM_THREADS) void km_apply(planes_t pl, int F, int k, int64_t n, const scaler_t<T> *__restrict__ sp,
                                                       const T *__restrict__ cenT, const T *__restrict__ csq, int32_t *__restrict__ out32,
                                                       T *__restrict__ dist, long long *__restrict__ partial, int64_t nchunks, int vec)
{
    constexpr int PXL = vt<T>::PXL;
    constexpr int TILE = KM_THREADS * PXL;
    constexpr bool DIST = (MODE & KA_DIST) != 0, SUM = (MODE & KA_SUM) != 0;
    extern __shared__ __align__(16) char smem[];
    const T *cen_s = reinterpret_cast<const T *>(smem);
    unsigned long long *S = reinterpret_cast<unsigned long long *>(smem + ka_cen_bytes<T>(MODE, KMAX, F));
    unsigned long long *myS = S + (size_t)(threadIdx.x & (KA_COPIES - 1)) * ka_cnt_stride(KMAX);
    const int rs = ka_row_stride(F);
    ka_fill_lds<T, MODE>(smem, KMAX, F, k, cenT);
    // csq in registers (uniform: SGPRs) as km_lloyd holds it, up to 64 of them: the 128 of 64 float64 norms do not fit beside the
    // rest (the labels-only form then ran out of registers: 20 B of scratch), so that case reads csq[j] where it is used
    constexpr bool CS_REGS = sizeof(T) * KMAX <= 256;
    T cs[CS_REGS ? KMAX : 1];
    if constexpr (CS_REGS) {
#pragma unroll
        for (int j = 0; j < KMAX; j++) cs[j] = csq[j];
    }
    auto csq_of = [&](int j) { if constexpr (CS_REGS) return cs[j]; else return csq[j]; };
    const int64_t chunk0 = (int64_t)blockIdx.x * km_chunk<T>();
    long long my_q = 0, my_ovf = 0;
    auto tile_body = [&](auto full_t, int64_t base) {
        constexpr bool FULL = decltype(full_t)::value;
        T x[FR][PXL];
#pragma unroll
        for (int f = 0; f < FR; f++) {
            if (f < F) load_pxf<T, FULL>(pl.p[f], base, n, x[f]);
            else {
#pragma unroll
                for (int p = 0; p < PXL; p++) x[f][p] = (T)0;
            }
        }
        T acc[KMAX][PXL];
#pragma unroll
        for (int j = 0; j < KMAX; j++)
#pragma unroll
            for (int p = 0; p < PXL; p++) acc[j][p] = (T)0;
#pragma unroll
        for (int f = 0; f < FR; f++) {
            if (f < F) {
                const T sc = sp->scale[f], mnv = sp->minv[f];
                T cj[KMAX];
#pragma unroll
                for (int j = 0; j < KMAX; j++) cj[j] = cenT[f * KMAX + j];
#pragma unroll
                for (int p = 0; p < PXL; p++) x[f][p] = scaled<T>(x[f][p], sc, mnv);
#pragma unroll
                for (int j = 0; j < KMAX; j++)
#pragma unroll
                    for (int p = 0; p < PXL; p++) acc[j][p] = tfma<T>(x[f][p], cj[j], acc[j][p]);
            }
        }
        int lab[PXL];
#pragma unroll
        for (int p = 0; p < PXL; p++) {
            T bd = tfma<T>((T)-2, acc[0][p], csq_of(0));
            int bl = 0;
#pragma unroll
            for (int j = 1; j < KMAX; j++) {
                if (j < k) {
                    T d = tfma<T>((T)-2, acc[j][p], csq_of(j));
                    if (d < bd) { bd = d; bl = j; }
                }
            }
            lab[p] = bl;
        }
        T sq[PXL], dv[PXL];
#pragma unroll
        for (int p = 0; p < PXL; p++) sq[p] = dv[p] = (T)0;
        if constexpr (MODE != 0) {
#pragma unroll
            for (int p = 0; p < PXL; p++) {
                const T *crow = cen_s + lab[p] * rs;
                T result = (T)0;
#pragma unroll
                for (int f = 0; f < FR; f += 4) {
                    if (f + 3 < F) {
                        const T d0 = x[f][p] - crow[f], d1 = x[f + 1][p] - crow[f + 1], d2 = x[f + 2][p] - crow[f + 2], d3 = x[f + 3][p] - crow[f + 3];
                        result = result + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            if (f + r < F) {
                                const T d = x[f + r][p] - crow[f + r];
                                result = result + d * d;
                            }
                    }
                }
                sq[p] = result;
                if constexpr (DIST) dv[p] = ka_sqrt<T>(result);
            }
        }
        ka_store<T, FULL>(out32, dist, DIST, base, n, vec, lab, dv);
        if constexpr (SUM) ka_tally<T, FULL>(myS, base, n, lab, sq, my_q, my_ovf);
    };
    for (int t = 0; t < KM_TILES_PER_CHUNK; t++) {
        const int64_t tbase = chunk0 + (int64_t)t * TILE;
        if (tbase >= n) break;
        const int64_t base = tbase + (int64_t)threadIdx.x * PXL;
        if (tbase + TILE <= n) tile_body(std::true_type{}, base);
        else tile_body(std::false_type{}, base);
    }
    if constexpr (SUM) ka_epilogue<T>(S, KMAX, my_q, my_ovf, partial, nchunks);
}

// feature-blocked form (33 <= F <= 64, and float64 with more than 32 clusters and F > 8): the dot products are carried across
// blocks of KM_FB planes in the same fma order; the blocks are walked a second time for sq (KM_FB is a multiple of four, so
// a group of four features never straddles two blocks).  The second read of a tile comes from the L2, as km_lloyd_blk's.
static_assert(KM_FB % 4 == 0, "km_apply_blk: a group of four features lies inside one block");
template <typename T, int KMAX, int MODE>
__global__ __launch_bounds__(KM_THREADS) void km_apply_blk(planes_t pl, int F, int k, int64_t n, const scaler_t<T> *__restrict__ sp,
                                                           const T *__restrict__ cenT, const T *__restrict__ csq, int32_t *__restrict__ out32,
                                                           T *__restrict__ dist, long long *__restrict__ partial, int64_t nchunks, int vec)
{
    constexpr int PXL = vt<T>::PXL;
    constexpr int TILE = KM_THREADS * PXL;
    constexpr bool DIST = (MODE & KA_DIST) != 0, SUM = (MODE & KA_SUM) != 0;
    extern __shared__ __align__(16) char smem[];
    const T *cen_s = reinterpret_cast<const T *>(smem);
    unsigned long long *S = reinterpret_cast<unsigned long long *>(smem + ka_cen_bytes<T>(MODE, KMAX, F));
    unsigned long long *myS = S + (size_t)(threadIdx.x & (KA_COPIES - 1)) * ka_cnt_stride(KMAX);
    const int rs = ka_row_stride(F);
    ka_fill_lds<T, MODE>(smem, KMAX, F, k, cenT);
    const int64_t chunk0 = (int64_t)blockIdx.x * km_chunk<T>();
    long long my_q = 0, my_ovf = 0;
    auto tile_body = [&](auto full_t, int64_t base) {
        constexpr bool FULL = decltype(full_t)::value;
        T acc[KMAX][PXL];
#pragma unroll
        for (int j = 0; j < KMAX; j++)
#pragma unroll
            for (int p = 0; p < PXL; p++) acc[j][p] = (T)0;
        for (int f0 = 0; f0 < F; f0 += KM_FB) {
            T x[KM_FB][PXL];
            load_block<T, FULL>(pl, F, f0, base, n, x);
#pragma unroll
            for (int jf = 0; jf < KM_FB; jf++) {
                const int f = f0 + jf;
                if (f < F) {
                    const T sc = sp->scale[f], mnv = sp->minv[f];
#pragma unroll
                    for (int p = 0; p < PXL; p++) x[jf][p] = scaled<T>(x[jf][p], sc, mnv);
#pragma unroll
                    for (int j = 0; j < KMAX; j++) {
                        const T cj = cenT[f * KMAX + j];
#pragma unroll
                        for (int p = 0; p < PXL; p++) acc[j][p] = tfma<T>(x[jf][p], cj, acc[j][p]);
                    }
                }
            }
        }
        int lab[PXL];
#pragma unroll
        for (int p = 0; p < PXL; p++) {
            T bd = tfma<T>((T)-2, acc[0][p], csq[0]);
            int bl = 0;
#pragma unroll
            for (int j = 1; j < KMAX; j++) {
                if (j < k) {
                    T d = tfma<T>((T)-2, acc[j][p], csq[j]);
                    if (d < bd) { bd = d; bl = j; }
                }
            }
            lab[p] = bl;
        }
        T sq[PXL], dv[PXL];
#pragma unroll
        for (int p = 0; p < PXL; p++) sq[p] = dv[p] = (T)0;
        if constexpr (MODE != 0) {
            for (int f0 = 0; f0 < F; f0 += KM_FB) {
                T x[KM_FB][PXL];
                load_block<T, FULL>(pl, F, f0, base, n, x);
#pragma unroll
                for (int jf = 0; jf < KM_FB; jf++) {
                    const int f = f0 + jf;
                    if (f < F) {
                        const T sc = sp->scale[f], mnv = sp->minv[f];
#pragma unroll
                        for (int p = 0; p < PXL; p++) x[jf][p] = scaled<T>(x[jf][p], sc, mnv);
                    }
                }
#pragma unroll
                for (int p = 0; p < PXL; p++) {
                    const T *crow = cen_s + lab[p] * rs + f0;
                    T result = sq[p];
#pragma unroll
                    for (int jf = 0; jf < KM_FB; jf += 4) {
                        if (f0 + jf + 3 < F) {
                            const T d0 = x[jf][p] - crow[jf], d1 = x[jf + 1][p] - crow[jf + 1], d2 = x[jf + 2][p] - crow[jf + 2],
                                    d3 = x[jf + 3][p] - crow[jf + 3];
                            result = result + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3);
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; r++)
                                if (f0 + jf + r < F) {
                                    const T d = x[jf + r][p] - crow[jf + r];
                                    result = result + d * d;
                                }
                        }
                    }
                    sq[p] = result;
                }
            }
            if constexpr (DIST) {
#pragma unroll
                for (int p = 0; p < PXL; p++) dv[p] = ka_sqrt<T>(sq[p]);
            }
        }
        ka_store<T, FULL>(out32, dist, DIST, base, n, vec, lab, dv);
        if constexpr (SUM) ka_tally<T, FULL>(myS, base, n, lab, sq, my_q, my_ovf);
    };
    for (int t = 0; t < KM_TILES_PER_CHUNK; t++) {
        const int64_t tbase = chunk0 + (int64_t)t * TILE;
        if (tbase >= n) break;
        const int64_t base = tbase + (int64_t)threadIdx.x * PXL;
        if (tbase + TILE <= n) tile_body(std::true_type{}, base);
        else tile_body(std::false_type{}, base);
    }
    if constexpr (SUM) ka_epilogue<T>(S, KMAX, my_q, my_ovf, partial, nchunks);
}

namespace {

// ---- K18: the sweep of a fitted model.  The same launch table as the Lloyd kernels (lloyd_form), times the four MODEs ----
template <typename T>
int launch_apply(rsseg_ctx *ctx, int mode, int64_t nchunks, planes_t pl, int F, int k, int KMAX, int64_t n, const scaler_t<T> *sp, const T *cenT,
                 const T *csq, int32_t *out32, T *dist, long long *partial, int vec)
{
    const size_t lds = ka_lds_bytes<T>(mode, KMAX, F);
    return with_kmax(KMAX, [&](auto kmax_c) {
        constexpr int KM = decltype(kmax_c)::value;
        return with_width(lloyd_form<T>(KMAX, F), [&](auto fr_c) -> int {
            constexpr int FR = decltype(fr_c)::value;
            const dim3 grid((unsigned)nchunks), block(KM_THREADS);
            auto go = [&](auto mode_c) -> int {
                constexpr int MODE = decltype(mode_c)::value;
                if constexpr (lloyd_form<T>(KM, FR) != FR) {
                    return RSSEG_OK;   // the table never picks this width for (T, KM): not instantiated
                } else if constexpr (FR == KM_BLOCKED) {
                    RSCHK(set_max_dyn_lds(ctx, (const void *)km_apply_blk<T, KM, MODE>, lds));
                    hipLaunchKernelGGL((km_apply_blk<T, KM, MODE>), grid, block, lds, ctx->stream, pl, F, k, n, sp, cenT, csq, out32, dist, partial,
                                       nchunks, vec);
                } else {
                    RSCHK(set_max_dyn_lds(ctx, (const void *)km_apply<T, KM, FR, MODE>, lds));
                    hipLaunchKernelGGL((km_apply<T, KM, FR, MODE>), grid, block, lds, ctx->stream, pl, F, k, n, sp, cenT, csq, out32, dist, partial,
                                       nchunks, vec);
                }
                return RSSEG_OK;
            };
            switch (mode) {
            case 0: return go(ic<0>());
            case KA_DIST: return go(ic<KA_DIST>());
            case KA_SUM: return go(ic<KA_SUM>());
            default: return go(ic<KA_DIST | KA_SUM>());
            }
        });
    });
}

template <typename T>
int kmeans_apply(rsseg_ctx *ctx, const void *const *d_planes, int F, int64_t n, int k, const double *centers, const double *scale,
                 const double *min_, int32_t *d_labels, void *d_dist, rsseg_kmeans_apply_info *info)
{
    const double t_start = now_ms();
    if (info) memset(info, 0, sizeof(*info));
    if (n > 0) {
        const int KMAX = km_kmax(k);
        const int mode = (d_dist ? KA_DIST : 0) | (info ? KA_SUM : 0);
        const int M = KMAX + 2;
        const int64_t nchunks = ceil_div64(n, km_chunk<T>());
        planes_t pl;
        memset(&pl, 0, sizeof(pl));
        for (int f = 0; f < F; f++) {
            if (!d_planes[f] || ((uintptr_t)d_planes[f] & 15)) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans: plane %d null or not 16-byte aligned", f);
            pl.p[f] = d_planes[f];
        }
        if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_dist & (sizeof(T) - 1))) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans_predict: output plane not aligned to its element");
        // the model as the kernels read it: scaler, transposed centres (cenT[f * KMAX + j]) and csq behind them, as kl_fill_cenT
        const size_t cen_count = (size_t)KMAX * RSSEG_MAX_FEATURES + KMAX;
        size_t off = 0;
        auto carve = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
        const size_t o_sp = carve(sizeof(scaler_t<T>));
        const size_t o_cen = carve(sizeof(T) * cen_count);
        const size_t up_bytes = off;   // the part that is uploaded in one copy
        const size_t o_part = carve(sizeof(long long) * (size_t)M * (size_t)nchunks);
        const size_t o_red = carve(sizeof(long long) * 2 * M);
        RSCHK(ws_reserve(ctx, off));
        RSCHK(pin_reserve(ctx, std::max<size_t>(up_bytes, sizeof(long long) * 2 * M)));
        char *ws = ctx->d_ws;
        memset(ctx->h_pin, 0, up_bytes);
        scaler_t<T> *hsp = (scaler_t<T> *)(ctx->h_pin + o_sp);
        T *hcen = (T *)(ctx->h_pin + o_cen), *hcsq = hcen + (size_t)KMAX * RSSEG_MAX_FEATURES;
        for (int f = 0; f < F; f++) {
            hsp->scale[f] = (T)scale[f];
            hsp->minv[f] = (T)min_[f];
        }
        for (int j = 0; j < k; j++) {
            T v = (T)0;
            for (int f = 0; f < F; f++) {
                const T c = (T)centers[(size_t)j * F + f];
                hcen[(size_t)f * KMAX + j] = c;
                v = std::fma(c, c, v);
            }
            hcsq[j] = v;
        }
        HIPCHK(ctx, hipMemcpyAsync(ws, ctx->h_pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
        const T *d_cen = (const T *)(ws + o_cen);
        long long *d_part = (long long *)(ws + o_part), *d_red = (long long *)(ws + o_red);
        const int vec = (((uintptr_t)d_labels & 15) == 0 ? 1 : 0) | (((uintptr_t)d_dist & 15) == 0 ? 2 : 0);
        {
            prof_scope ps(ctx, "kmeans_apply");
            RSCHK(launch_apply<T>(ctx, mode, nchunks, pl, F, k, KMAX, n, (const scaler_t<T> *)(ws + o_sp), d_cen, d_cen + (size_t)KMAX * RSSEG_MAX_FEATURES,
                                  d_labels, (T *)d_dist, d_part, vec));
            HIPCHK(ctx, hipGetLastError());
            if (info) {
                RSCHK(km_reduce_cols_launch(ctx, d_part, nchunks, M, d_red));
            }
        }
        // the upload has to have left the pinned area before the read-back lands in it
        HIPCHK(ctx, rs_sync(ctx));
        if (info) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_pin, d_red, sizeof(long long) * 2 * M, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, rs_sync(ctx));
            const long long *r = (const long long *)ctx->h_pin;
            for (int j = 0; j < k; j++) info->counts[j] = (int64_t)limbs(r[2 * j], r[2 * j + 1]);
            info->overflow = limbs(r[2 * (KMAX + 1)], r[2 * (KMAX + 1) + 1]) != 0;
            info->inertia = info->overflow ? (double)INFINITY : fixed_to_T<double>(limbs(r[2 * KMAX], r[2 * KMAX + 1]));
        }
    }
    if (info) info->ms = now_ms() - t_start;
    return RSSEG_OK;
}

}  // namespace

extern "C" int rsseg_kmeans_predict(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n_local, int k, const double *centers,
                                    const double *scale, const double *min_, int32_t *d_labels, void *d_dist, rsseg_kmeans_apply_info *info)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || F < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans: no feature planes");
    if (k < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans: n_clusters=%d must be >= 1", k);
    if (F > RSSEG_MAX_FEATURES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "kmeans: %d feature planes, the kernels take at most %d", F, RSSEG_MAX_FEATURES);
    if (k > RSSEG_MAX_CLUSTERS) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "kmeans: n_clusters=%d, the kernels take at most %d", k, RSSEG_MAX_CLUSTERS);
    if (n_local < 0 || (n_local > 0 && !d_labels)) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans: bad n_local / labels");
    if (dtype != RSSEG_F32 && dtype != RSSEG_F64) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans: dtype must be RSSEG_F32 or RSSEG_F64");
    if (!centers || !scale || !min_) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans_predict: the model (centers, scale, min_) is missing");
    auto check = [&](const char *what, const double *v, int count) -> int {
        for (int i = 0; i < count; i++) {
            if (!std::isfinite(v[i])) return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans_predict: %s[%d] is not finite", what, i);
            if (dtype == RSSEG_F32 && (double)(float)v[i] != v[i])
                return rs_fail(ctx, RSSEG_ERR_INVALID, "kmeans_predict: %s[%d] is not a float32 value: a model fitted in float64 cannot be applied to float32 planes", what, i);
        }
        return RSSEG_OK;
    };
    RSCHK(check("centers", centers, k * F));
    RSCHK(check("scale", scale, F));
    RSCHK(check("min_", min_, F));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (dtype == RSSEG_F32) return kmeans_apply<float>(ctx, d_planes, F, n_local, k, centers, scale, min_, d_labels, d_dist, info);
    return kmeans_apply<double>(ctx, d_planes, F, n_local, k, centers, scale, min_, d_labels, d_dist, info);
}
