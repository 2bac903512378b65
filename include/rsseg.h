/*
 * rsseg.h — C ABI of librsseg_hip.so: MI355X (gfx950) kernels for the per-pixel
 * feature-extraction -> clustering / classification path of beilsme/rs-image-segmentation, the stages around it
 * (preprocessing, accuracy assessment, class-map clean-up) and, beyond the reference, the geometric correction from
 * ground control points that its stage 1 only stubs (rsseg_warp_poly).
 *
 * The reference has no FFI: its boundary for this path is a set of NumPy-in / NumPy-out Python
 * functions.  Each entry point below names the reference function (file:line,
 * relative to the reference repository) whose arithmetic it replaces; the Python mirror of those
 * functions (rs-image-segmentation_amd/modules/...) binds this header through ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - Pointers named d_* are DEVICE addresses (e.g. torch tensor .data_ptr()); all others are host.
 *   - Rasters are band/feature-PLANAR: one contiguous (H*W) plane per band, row-major.
 *   - Every call is synchronous with respect to its results: it returns after the work it
 *     enqueued on the context's stream has completed, unless stated otherwise.
 *   - Return value: 0 = RSSEG_OK, negative = error (rsseg_last_error gives the text).  Never aborts.
 *   - One caller thread per context (the reference is single-threaded).
 *   - Multi-GPU: one context per process/GPU; a context given world > 1 calls the registered
 *     all-reduce hook on small device buffers (RCCL through torch.distributed on the host side).
 */
#ifndef RSSEG_H
#define RSSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSSEG_OK 0
#define RSSEG_ERR_INVALID (-1)   /* bad argument (ValueError on the Python side) */
#define RSSEG_ERR_HIP (-2)       /* HIP runtime error */
#define RSSEG_ERR_NOMEM (-3)
#define RSSEG_ERR_COMM (-4)      /* all-reduce hook failed */
#define RSSEG_ERR_UNSUPPORTED (-5)

#define RSSEG_F32 0
#define RSSEG_F64 1
#define RSSEG_I64 2
/* integer label planes (rsseg_confusion_counts) and DN planes (rsseg_preprocess_u8) */
#define RSSEG_U8 3
#define RSSEG_I16 4
#define RSSEG_U16 5
#define RSSEG_I32 6

#define RSSEG_SUM 0
#define RSSEG_MIN 1
#define RSSEG_MAX 2

#define RSSEG_BORDER_REFLECT 0     /* cv2.BORDER_REFLECT      fedcba|abcdefgh|hgfedcb */
#define RSSEG_BORDER_REFLECT101 1  /* cv2.BORDER_REFLECT_101  gfedcb|abcdefgh|gfedcba */

#define RSSEG_MAX_FEATURES 64
#define RSSEG_MAX_CLUSTERS 64
#define RSSEG_MAX_RANKS 16

typedef struct rsseg_ctx rsseg_ctx;

/* All-reduce hook: reduce `count` elements of `dtype` (RSSEG_F32/F64/I64) with `op`
 * (RSSEG_SUM/MIN/MAX) IN PLACE at byte offset `offset` of the communication buffer registered with
 * rsseg_ctx_set_comm, across all ranks, ordered after the work already enqueued on the context's
 * stream AND before the work the library enqueues on that stream after the hook has returned: inside
 * rsseg_kmeans_fit_predict a kernel leaves its partials in the buffer, the hook is called, and the next kernel reads
 * the reduced values, without the host waiting in between (ncclAllReduce on the context's stream, or
 * torch.distributed.all_reduce with that stream current, give exactly this; a hook that synchronises is also
 * correct).  Every rank calls the hook the same number of times with the same arguments.  Returns 0 on success. */
typedef int (*rsseg_allreduce_fn)(void *user, int64_t offset, int64_t count, int dtype, int op);

/* ---- context ---------------------------------------------------------------------------- */
/* stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream), or NULL for a non-blocking
 * stream owned by the context.  The library orders its work on THAT stream only: an input plane still being written
 * by work on another stream must be complete before the call.  A host whose producers run on the legacy default
 * stream (torch's default) passes hipStreamLegacy ((hipStream_t)1), as rsseg/runtime.py does. */
int rsseg_ctx_create(int device, void *stream, rsseg_ctx **out);
void rsseg_ctx_destroy(rsseg_ctx *ctx);
const char *rsseg_last_error(const rsseg_ctx *ctx);
const char *rsseg_version(void);
/* While on, the spectral-index call (7 index planes), the two bilinear-upsample calls (1 plane) and the PCA call
 * (n_components planes) also reduce the minimum and maximum of every plane they write, NaN counted
 * as 0 (what KMeans' MinMaxScaler sees); rsseg_ctx_last_minmax returns them, by output index (at most 16), until the next such call. */
int rsseg_ctx_collect_minmax(rsseg_ctx *ctx, int on);
int rsseg_ctx_last_minmax(rsseg_ctx *ctx, int plane, double *mn, double *mx);
/* Asynchronous mode: entry points whose results stay on the device (normalize, indices, quantize, glcm, resize,
 * window operators, forest_predict) return right after enqueueing on the context's stream; rsseg_ctx_sync waits.
 * Used to run the VALU-bound GLCM on a second stream beside the HBM-bound passes (rsseg/pipeline.py). */
int rsseg_ctx_set_async(rsseg_ctx *ctx, int on);
int rsseg_ctx_sync(rsseg_ctx *ctx);
/* d_comm: device buffer of comm_bytes (>= 1 MiB) owned by the caller, visible to the hook.  The hook is called whenever one is
 * installed together with a buffer — also with world == 1, where the reduction is the identity: that is how a one-GPU box
 * runs every collective of a step through RCCL.  fn == NULL with world == 1 removes it. */
int rsseg_ctx_set_comm(rsseg_ctx *ctx, int rank, int world, rsseg_allreduce_fn fn, void *user,
                       void *d_comm, size_t comm_bytes);

/* The same with RCCL driven by the library itself (no callback, no Python in the loop): every reduction becomes an
 * ncclAllReduce, in place in the communication buffer, enqueued on the context's stream.  Rank 0 obtains the 128-byte
 * ncclUniqueId with rsseg_rccl_unique_id and the host hands it to every rank by whatever means it has (torch.distributed's
 * store, MPI, a file); then EVERY rank calls rsseg_ctx_set_comm_rccl (collective: ncclCommInitRank).  librccl_path names
 * the librccl.so the process uses (torch ships one in torch/lib; NULL: "librccl.so.1" from the loader path); it is
 * dlopen()ed, not linked.  d_comm may be NULL: the library then owns a 4 MiB buffer.  world == 1 is allowed (identity
 * reductions through RCCL).  rsseg_ctx_set_comm or rsseg_ctx_destroy release the communicator.
 * (This is the form SURVEY.md 8b sketched as rsseg_ctx_create(device, rank, world, ncclUniqueId*).) */
#define RSSEG_RCCL_ID_BYTES 128
int rsseg_rccl_unique_id(const char *librccl_path, void *id_out);
int rsseg_ctx_set_comm_rccl(rsseg_ctx *ctx, int rank, int world, const void *unique_id, const char *librccl_path, void *d_comm,
                            size_t comm_bytes);

/* One reduction over whatever communication path is installed (callback or RCCL), as the library's own kernels use it:
 * `count` elements of `dtype` at byte `offset` of the communication buffer, in place, enqueued on the context's stream
 * (no host wait).  Without a communication path (one rank) it is the identity.  For hosts that keep cross-rank values of
 * their own in the buffer, and for testing a path's stream ordering. */
int rsseg_ctx_allreduce(rsseg_ctx *ctx, int64_t offset, int64_t count, int dtype, int op);

/* Per-kernel timing (HIP events on the context's stream, around each launch of the named
 * kernel family).  Used by bench.py for the roofline object.  name: "glcm", "lloyd", "indices", "normalize", "quantize", "range",
 * "select", "kpp", "moment" (KMeans' column means), "labels" (uint8 -> int32 label plane), "box" (one plane), "ctxmean" (several planes per launch), "morph", "filt_max" / "filt_write" (the two passes
 * of Sobel / Laplacian), "project", "indices_project" (the fused pass of rsseg_indices_pca_*), "gram", "forest", "resize", "eval_range" / "eval_table"
 * (the two passes of rsseg_confusion_counts), "pre_range" / "pre_stretch" (the two passes of rsseg_preprocess_u8), and "allreduce" (host wall time of the hook calls). */
/* Number of times the library has made the host wait for the context's stream since the last reset (every result
 * read-back, every all-reduce staged through the host): what a step costs in launch-pipeline bubbles. */
int rsseg_ctx_host_syncs(rsseg_ctx *ctx, int reset, int64_t *count);
int rsseg_prof_enable(rsseg_ctx *ctx, int on);
int rsseg_prof_reset(rsseg_ctx *ctx);
int rsseg_prof_get(rsseg_ctx *ctx, const char *name, double *total_ms, int64_t *launches);

/* ---- K1: exact order statistics ------------------------------------------------------- */
/* Replaces the partition inside np.percentile (modules/features/indices.py:38-39) and
 * np.nanmedian / np.nanpercentile of RobustScaler (indices.py:230-231).
 * For each r in ranks[0..nranks) (0-based positions in the ascending order of ALL n_global
 * values, NaNs last) writes the value at that position to out_values.  n_nan_out receives the
 * global NaN count.  The interpolation between neighbouring order statistics is done by the
 * caller exactly as NumPy does (host arithmetic on two scalars). */
int rsseg_order_stats_f32(rsseg_ctx *ctx, const float *d_x, int64_t n_local, const int64_t *ranks,
                          int nranks, float *out_values, int64_t *n_nan_out);
/* The same for up to 8 planes of equal length at once (ranks: [nplanes][nranks], out_values: [nplanes][nranks],
 * n_nan_out: [nplanes]): the planes advance pass by pass together, so a group costs three host synchronisations
 * and three all-reduces instead of three per plane.  With world > 1 the communication buffer must hold
 * nplanes * 262 208 bytes. */
int rsseg_order_stats_multi_f32(rsseg_ctx *ctx, const float *const *d_planes, int nplanes, int64_t n_local,
                                const int64_t *ranks, int nranks, float *out_values, int64_t *n_nan_out);

/* The same for 8-bit planes (one byte per pixel; the TM tiles the reference reads are uint8 digital numbers,
 * modules/features/preprocessing.py:117-118, which scripts/2_feature_extraction.py:156 widens with .astype(np.float32)):
 * one 256-bin pass, the values come back as float32 like np.percentile of the widened band would give them. */
int rsseg_order_stats_multi_u8(rsseg_ctx *ctx, const uint8_t *const *d_planes, int nplanes, int64_t n_local,
                               const int64_t *ranks, int nranks, float *out_values, int64_t *n_nan_out);

/* ---- K2: percentile normalisation + spectral indices ------------------------------------ */
/* robust_normalize (indices.py:25-48), elementwise part: clip to [lo,hi], (x-lo)/(hi-lo+1e-10)
 * in float32.  d_out may alias d_x. */
int rsseg_normalize_f32(rsseg_ctx *ctx, const float *d_x, int64_t n, float lo, float hi, float *d_out);

/* Fused robust_normalize of the five bands the indices read + calculate_ndvi / evi / msavi /
 * ndwi / mndwi / ndbi / bsi (indices.py:50-203; call order scripts/2_feature_extraction.py:63-73).
 * d_bands[5] = raw blue, green, red, nir, swir1 planes; lohi[10] = (lo,hi) per band.
 * d_out[7] = ndvi, evi, msavi, ndwi, mndwi, ndbi, bsi planes (any may be NULL = not wanted).
 * d_norm[5] (optional, entries may be NULL) receive the normalised bands.
 * If lohi == NULL the bands are taken as already normalised. */
int rsseg_spectral_indices_f32(rsseg_ctx *ctx, const float *const *d_bands, int64_t n, const float *lohi,
                               float *const *d_out, float *const *d_norm);
/* The same with calculate_evi's coefficients evi_coef[4] = {L, C1, C2, G} (indices.py:73; NULL = the defaults 1, 6, 7.5, 2.5). */
int rsseg_spectral_indices_evi_f32(rsseg_ctx *ctx, const float *const *d_bands, int64_t n, const float *lohi,
                                   float *const *d_out, float *const *d_norm, const float *evi_coef);

/* The same on 8-bit band planes: bit for bit the result of the float32 entry point on the widened planes (the
 * normalisation of a byte is a 256-entry table filled with the float path's own operations); 5 B/px read instead of 20. */
int rsseg_spectral_indices_evi_u8(rsseg_ctx *ctx, const uint8_t *const *d_bands, int64_t n, const float *lohi,
                                  float *const *d_out, float *const *d_norm, const float *evi_coef);

/* ---- K3: PCA ------------------------------------------------------------------------------ */
/* perform_pca (indices.py:205-246): RobustScaler transform x' = (float)((double)(x - center) /
 * scale) applied on the fly, then mean / Gram accumulation (exact), covariance, symmetric
 * eigen-decomposition, sign convention of sklearn's svd_flip, projection to n_components planes.
 * d_bands[nb]: normalised band planes; center[nb] (float32 medians) and scale[nb] (float64 IQRs)
 * come from K1 + host interpolation; pass center = NULL for no scaling.
 * Outputs (host): components (n_components x nb, row-major, float32), explained_variance_ratio
 * (n_components), mean (nb), explained_variance (n_components). d_out[n_components]: projected planes.
 * Value range: the sums are exact in quanta of 2^-Q, Q = min(38, 48 - ceil(log2(bound^2))) with bound the largest
 * |scaled value| of the fit (1 for normalised bands, measured otherwise).  Q < -19 (bound above about 1e10) is
 * refused with RSSEG_ERR_UNSUPPORTED: the band sums share the quantum of the squares, and below it the mean is
 * rounded more coarsely than scikit-learn's float32 steps round it. */
int rsseg_pca_fit_transform_f32(rsseg_ctx *ctx, const float *const *d_bands, int nb, int64_t n_local,
                                const float *center, const double *scale, int n_components,
                                float *const *d_out, float *components, float *explained_variance_ratio,
                                float *mean, float *explained_variance);
/* The same on RAW bands: each value first goes through robust_normalize with lohi[2*b], lohi[2*b+1] (np.percentile 2 /
 * 98 of band b) — the arithmetic of rsseg_normalize_f32 — so the normalised planes need not exist in memory. */
int rsseg_pca_fit_transform_raw_f32(rsseg_ctx *ctx, const float *const *d_bands, int nb, int64_t n_local, const float *lohi,
                                    const float *center, const double *scale, int n_components, float *const *d_out,
                                    float *components, float *explained_variance_ratio, float *mean,
                                    float *explained_variance);

/* The same with the FIT restricted to the pixels [fit_off, fit_off + fit_n) of the planes while all n_local pixels are
 * projected: a rank of a row-sharded raster passes its stripe plus halo rows (the 7x7 context mean of the first
 * component needs 3 rows either side, indices.py:770) and fits on the rows it owns.  lohi may be NULL (bands already
 * normalised), center / scale may be NULL (no RobustScaler). */
int rsseg_pca_fit_transform_ext_f32(rsseg_ctx *ctx, const float *const *d_bands, int nb, int64_t n_local, int64_t fit_off,
                                    int64_t fit_n, const float *lohi, const float *center, const double *scale, int n_components,
                                    float *const *d_out, float *components, float *explained_variance_ratio, float *mean,
                                    float *explained_variance);
/* rsseg_pca_fit_transform_ext_f32 on 8-bit band planes (bit for bit the float32 result on the widened planes). */
int rsseg_pca_fit_transform_ext_u8(rsseg_ctx *ctx, const uint8_t *const *d_bands, int nb, int64_t n_local, int64_t fit_off,
                                   int64_t fit_n, const float *lohi, const float *center, const double *scale, int n_components,
                                   float *const *d_out, float *components, float *explained_variance_ratio, float *mean,
                                   float *explained_variance);
/* The spectral indices AND the PCA of the same raw bands in two passes instead of three: the fit (Gram pass) as in
 * rsseg_pca_fit_transform_ext_*, then ONE pass that writes the seven index planes d_idx[7] (ndvi, evi, msavi, ndwi, mndwi,
 * ndbi, bsi; entries may be NULL), optionally the normalised bands d_norm[5] (may be NULL, entries may be NULL) and the
 * n_components projected planes d_pc — the values rsseg_spectral_indices_evi_* and rsseg_pca_fit_transform_ext_* return,
 * bit for bit (calculate_* of indices.py:50-203 and perform_pca of :205-246 on the same robust-normalised bands, as
 * scripts/2_feature_extraction.py:63-78 calls them).  d_bands[0..4] = blue, green, red, nir, swir1; lohi[2 * nb] is required.
 * d_q (optional): the texture chain's input in the same pass — rsseg_normalize_quantize_u8 of the normalised NIR band
 * (band 3) with the percentiles q_lo, q_hi of THAT normalised band and the multiplier q_mult (levels - 1 or 255):
 * calculate_glcm_features re-normalises the band it receives and truncates it to uint8 (indices.py:265-268).
 * With rsseg_ctx_collect_minmax on, rsseg_ctx_last_minmax(0..6) are the indices' extrema, (7 + c) the components'. */
int rsseg_indices_pca_f32(rsseg_ctx *ctx, const float *const *d_bands, int nb, int64_t n_local, int64_t fit_off, int64_t fit_n,
                          const float *lohi, const float *center, const double *scale, int n_components, const float *evi_coef,
                          float *const *d_idx, float *const *d_norm, float *const *d_pc, uint8_t *d_q, float q_lo, float q_hi,
                          float q_mult, float *components, float *explained_variance_ratio, float *mean, float *explained_variance);
int rsseg_indices_pca_u8(rsseg_ctx *ctx, const uint8_t *const *d_bands, int nb, int64_t n_local, int64_t fit_off, int64_t fit_n,
                         const float *lohi, const float *center, const double *scale, int n_components, const float *evi_coef,
                         float *const *d_idx, float *const *d_norm, float *const *d_pc, uint8_t *d_q, float q_lo, float q_hi,
                         float q_mult, float *components, float *explained_variance_ratio, float *mean, float *explained_variance);
/* Errors of the PCA entry points: RSSEG_ERR_INVALID "Input X contains NaN." / "... infinity" (sklearn's PCA raises
 * ValueError on such input, sklearn/utils/validation.py); bands that are not robust-normalised are range-checked
 * with one extra pass so that the exact fixed-point accumulation fits any finite input (raw DN, reflectances). */

/* ---- K4/K5: GLCM texture + bilinear upsample ------------------------------------------- */
/* calculate_glcm_features (indices.py:248-318), window loop: d_q is the quantised uint8 plane
 * ((band*(levels-1)).astype(uint8), :268), H x W.  Writes the five property maps
 * (contrast, dissimilarity, homogeneity, energy, correlation), each ((H-win)/step+1) x
 * ((W-win)/step+1) float32, mean over the 4 angles (0, 45, 90, 135 degrees, distance 1),
 * symmetric + normalised co-occurrence. Any of d_props[i] may be NULL.  levels 2..256 (65..256: win <= 255);
 * RSSEG_ERR_UNSUPPORTED for levels > 256. */
int rsseg_glcm_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int levels, int win, int step,
                  float *const *d_props);
/* The same for any list of graycomatrix (distance, angle) entries (indices.py:288-290): offsets holds n pairs (dr, dc) in
 * entry order (distance-major, angle-minor), dr = round(sin(angle) * distance), dc = round(cos(angle) * distance)
 * (rsseg/pipeline.py::glcm_offset_plan).  Pixel (r, c) pairs with (r + dr, c + dc) inside the window; an offset that
 * leaves the window gives the empty matrix, whose properties are (0, 0, 0, 0, 1).  Each map is the float32 of the plain
 * mean over the n entries; each entry's properties come from exact integer statistics in float64 (k4_glcm_offsets.hip).
 * The default list (0,1), (1,1), (1,0), (1,-1) is rsseg_glcm_u8 itself, bit for bit.  RSSEG_ERR_UNSUPPORTED: levels > 256;
 * a non-default list with win > 255; more than 512 entries or 64 distinct offsets (o and -o are one offset). */
int rsseg_glcm_offsets_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int levels, int win, int step,
                          const int32_t *offsets, int n, float *const *d_props);
/* float32 plane in [0,1] -> uint8 by truncation of x*mult (indices.py:268, 415, 458). */
int rsseg_quantize_u8(rsseg_ctx *ctx, const float *d_x, int64_t n, float mult, uint8_t *d_q);
/* robust_normalize(x) with the given percentiles, then the truncation of rsseg_quantize_u8, in one pass (the texture
 * functions re-normalise the band they receive before quantising it, indices.py:265-268, 412-415). */
int rsseg_normalize_quantize_u8(rsseg_ctx *ctx, const float *d_x, int64_t n, float lo, float hi, float mult, uint8_t *d_q);
/* uint8 plane -> float32 of (uint8 / 255.0 in float64): the value sklearn sees for the morphological members
 * (features[...] = gradient / 255.0, indices.py:436-440; float32 cast sklearn/ensemble/_forest.py:640). */
int rsseg_u8_to_unit_f32(rsseg_ctx *ctx, const uint8_t *d_q, int64_t n, float *d_out);
/* uint8 plane -> float32 plane, exact: band.astype(np.float32) of an 8-bit raster (scripts/2_feature_extraction.py:156), for the
 * entry points that have no 8-bit form. */
int rsseg_u8_to_f32(rsseg_ctx *ctx, const uint8_t *d_q, int64_t n, float *d_out);
/* cv2.resize(src, (dw, dh), interpolation=INTER_LINEAR) for float32 (indices.py:308). */
int rsseg_resize_bilinear_f32(rsseg_ctx *ctx, const float *d_src, int sh, int sw, float *d_dst, int dh, int dw);
/* Row-striped form for sharded rasters: d_src holds rows [src_row0, src_row0 + sh_local) of a source sh rows tall,
 * d_dst receives rows [dst_row0, dst_row0 + dh_local) of the dh x dw result; identical values to the un-sharded call. */
int rsseg_resize_bilinear_rows_f32(rsseg_ctx *ctx, const float *d_src, int sh_local, int sw, int src_row0, int sh,
                                   float *d_dst, int dh_local, int dw, int dst_row0, int dh);

/* The same for nplanes (<= 8) source maps of one shape in ONE launch (the five GLCM property maps, indices.py:307-310);
 * with rsseg_ctx_collect_minmax on, rsseg_ctx_last_minmax(plane) returns the extrema of each. */
int rsseg_resize_bilinear_rows_multi_f32(rsseg_ctx *ctx, const float *const *d_src, int nplanes, int sh_local, int sw, int src_row0, int sh,
                                         float *const *d_dst, int dh_local, int dw, int dst_row0, int dh);

/* ---- K6/K7/K8: window operators ---------------------------------------------------------- */
/* Every operator exists in a ROWS form for row-sharded rasters: the plane holds Hin rows, rows
 * [y0, y1) are produced into a compact (y1 - y0) x W output.  edges bit 0 / bit 1 say that row 0 / row Hin - 1 is the
 * image's first / last row, where the operator's border rule applies; a side that is not an image edge must carry
 * R = k/2 halo rows (2R for opening / closing), otherwise RSSEG_ERR_INVALID.  The plain forms are rows (0, H), edges 3.
 * The stripes of a sharded raster get exactly the rows of the un-sharded result. */
/* cv2.boxFilter(normalize=True) / cv2.blur for float32 (indices.py:770-771, 537, 541): k x k mean, k in {3,5,7,9},
 * float64 sums in a fixed order (row sums left to right, then top to bottom), border RSSEG_BORDER_*.  If square != 0
 * the input is squared (float32) first (blur(band*band), indices.py:541). */
int rsseg_box_mean_f32(rsseg_ctx *ctx, const float *d_x, int H, int W, int k, int border, int square,
                       float *d_out);
/* The same for nplanes (<= 8) planes of equal shape in ONE launch (add_spatial_context loops over 7 channels). */
int rsseg_box_mean_rows_f32(rsseg_ctx *ctx, const float *const *d_x, int nplanes, int Hin, int W, int y0, int y1, int edges,
                            int k, int border, int square, float *const *d_out);
/* std_dev_scale_k (indices.py:537-548): sqrt(max(blur(x*x) - blur(x)^2, 0)), REFLECT_101. */
int rsseg_local_std_f32(rsseg_ctx *ctx, const float *d_x, int H, int W, int k, float *d_out);
/* variance_scale_k (indices.py:541-544): max(blur(x*x) - blur(x)^2, 0), REFLECT_101 (rsseg_local_std_f32 without the sqrt). */
int rsseg_local_var_f32(rsseg_ctx *ctx, const float *d_x, int H, int W, int k, float *d_out);
/* rows form of both: variance != 0 selects variance_scale_k */
int rsseg_local_std_rows_f32(rsseg_ctx *ctx, const float *d_x, int Hin, int W, int y0, int y1, int edges, int k, int variance,
                             float *d_out);
/* cv2.morphologyEx(MORPH_GRADIENT, ones(k,k)) on uint8 (indices.py:422, 433); output uint8. */
int rsseg_morph_gradient_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int k, uint8_t *d_out);
/* cv2.erode / cv2.dilate / cv2.morphologyEx(MORPH_OPEN | MORPH_CLOSE | MORPH_GRADIENT) with ones(k,k) on uint8
 * (calculate_morphological_features, indices.py:421-433): k in {3,5,7}, default border (out-of-image taps never win),
 * opening = dilate(erode(x)), closing = erode(dilate(x)).  Output uint8 (the caller divides by 255.0, :436-440). */
#define RSSEG_MORPH_ERODE 0
#define RSSEG_MORPH_DILATE 1
#define RSSEG_MORPH_OPEN 2
#define RSSEG_MORPH_CLOSE 3
#define RSSEG_MORPH_GRADIENT 4
int rsseg_morph_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int k, int op, uint8_t *d_out);
int rsseg_morph_rows_u8(rsseg_ctx *ctx, const uint8_t *d_q, int Hin, int W, int y0, int y1, int edges, int k, int op,
                        uint8_t *d_out);
/* 'laplacian' of calculate_filter_responses (indices.py:472-474): cv2.Laplacian(u8, CV_32F) (3x3 cross, REFLECT_101)
 * / 255.0, then (l - min) / (max - min + 1e-10) in float32.  Two passes over the uint8 plane (extrema, then the
 * normalised write); the global min / max of the produced rows go through the all-reduce hook. */
int rsseg_laplacian_norm_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, float *d_out);
int rsseg_laplacian_norm_rows_u8(rsseg_ctx *ctx, const uint8_t *d_q, int Hin, int W, int y0, int y1, int edges, float *d_out);
/* sobel_mag (indices.py:477-480): 3x3 Sobel x/y of the uint8 plane as float32 / 255, magnitude,
 * divided by (global max + 1e-10).  Two passes as above; the global max goes through the all-reduce hook. */
int rsseg_sobel_mag_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, float *d_out);
int rsseg_sobel_mag_rows_u8(rsseg_ctx *ctx, const uint8_t *d_q, int Hin, int W, int y0, int y1, int edges, float *d_out);

/* ---- K17: correlation with a bank of float32 kernels (calculate_gabor_features, indices.py:346-399) ------------ */
/* cv2.filter2D(u8, CV_32F, kern)'s direct path for nf kernels of one odd size ksize <= 15: out[f][y][x] = sum over i, then
 * j (row-major), of taps[f][i][j] * u8[y + i - m][x + j - m], m = ksize / 2, BORDER_REFLECT_101 (reflected repeatedly on a
 * plane smaller than m; an axis of one element reads that element), started from +0, one rounded float32 multiply and one
 * rounded float32 add per tap, subnormals kept.  h_taps: nf * ksize * ksize floats on the host; d_out: nf planes of H * W
 * float32, 16-byte aligned, not the input; h_minmax (host, 2 * nf, may be NULL): {min, max} of every plane.  Up to 8
 * kernels share one launch and one staging of the plane.  Whole plane on one device: there is no rows form.
 * RSSEG_ERR_INVALID, with a text: ksize even or outside 1..15, nf < 1, H or W < 1, a NaN or infinite tap.
 * Supported tap range: the sum of |tap| of a kernel times 255 must stay finite in float32 (sum |tap| < 1.3e36; the Gabor taps
 * are <= 1).  Finite taps beyond that are not refused: a response overflows to +-inf, inf - inf gives NaN, and the extrema
 * (which count NaN as 0) and the normalised planes are then meaningless, without a report. */
int rsseg_correlate_u8_f32(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, const float *h_taps, int ksize, int nf, float *d_out,
                           float *h_minmax);
/* the same, then every plane min-max normalised in place: (r - min) / (max - min + 1e-10) in float32 (indices.py:395), the
 * roundings of rsseg_laplacian_norm_u8 and a true division; a constant plane gives zeros. */
int rsseg_filter_bank_norm_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, const float *h_taps, int ksize, int nf, float *d_out);
/* the output tile (rows, columns) one workgroup of K17 owns: tests place their shapes and seams by it */
void rsseg_correlate_tile(int *tile_h, int *tile_w);

/* ---- K9/K10: KMeans ------------------------------------------------------------------------ */
typedef struct rsseg_kmeans_info {
    int32_t n_iter;
    int32_t relocated;            /* empty-cluster relocations performed */
    double tol;                   /* tol * mean(var) actually used */
    double scale[RSSEG_MAX_FEATURES];
    double min[RSSEG_MAX_FEATURES];
    double mean[RSSEG_MAX_FEATURES];
    int64_t init_indices[RSSEG_MAX_CLUSTERS]; /* global pixel index of each k-means++ seed */
    double ms_init;               /* wall milliseconds: scaler + k-means++ */
    double ms_lloyd;              /* wall milliseconds: Lloyd iterations */
} rsseg_kmeans_info;

/* unsupervised_kmeans_classification (modules/features/extract.py:568-579): NaN->0, MinMaxScaler,
 * KMeans(n_clusters, random_state=seed, n_init=1, init='k-means++', max_iter, tol).fit_predict.
 * d_planes[F]: feature planes, all float32 (dtype RSSEG_F32) or all float64 (RSSEG_F64), n_local
 * pixels each (this rank's stripe; ranks hold consecutive stripes in rank order).
 * d_labels: int32[n_local], cluster ids 0..k-1.  centers (host, k*F doubles, scaled-and-centred
 * space + mean added back, like cluster_centers_). */
int rsseg_kmeans_fit_predict(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n_local,
                             int k, uint32_t seed, int max_iter, double tol, int32_t *d_labels,
                             double *centers, rsseg_kmeans_info *info);
/* The same when the caller already knows this rank's minimum and maximum of every plane (NaN counted as 0), e.g. from
 * rsseg_ctx_last_minmax: the MinMaxScaler pass over the planes is skipped (the extrema are still all-reduced). */
int rsseg_kmeans_fit_predict_mm(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n_local, int k,
                                uint32_t seed, int max_iter, double tol, int32_t *d_labels, double *centers,
                                rsseg_kmeans_info *info, const double *local_min, const double *local_max);

/* K18: a FITTED model applied to planes it may not have been fitted on (MinMaxScaler.transform + KMeans.predict): labels,
 * on request the distance of every pixel to the centre of its label (d_dist) and the scene's per-cluster pixel counts and
 * inertia (info).  Inertia is the exact sum of the squared distances rounded to 2^-40; a pixel whose squared distance
 * reaches 2^23 / chunk - 2^-41 (512 for float32, 1024 for float64) is left out of it and raises `overflow`: the call then
 * still returns RSSEG_OK with inertia = +inf, and labels, counts and distances stay valid.
 * The summary is this context's own: with a communicator installed the call reduces NOTHING; a sharded caller adds the
 * counts and the inertia of its ranks itself.  n_local == 0 is legal (zero counts, inertia 0). */
typedef struct rsseg_kmeans_apply_info {
    int64_t counts[RSSEG_MAX_CLUSTERS];
    double  inertia;      /* +inf when overflow */
    int32_t overflow;
    double  ms;           /* wall milliseconds of the call */
} rsseg_kmeans_apply_info;

int rsseg_kmeans_predict(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n_local, int k,
                         const double *centers,  /* host, k*F: cluster_centers_ as the fit returns them */
                         const double *scale, const double *min_,   /* host, F each: rsseg_kmeans_info.scale / .min */
                         int32_t *d_labels, void *d_dist /* NULL or T[n_local] */,
                         rsseg_kmeans_apply_info *info /* NULL: no summary */);

/* ---- K19: valid masks and order-preserving compaction ------------------------------------------ */
/* A scene with a nodata collar and holes is classified on its valid pixels only: build a mask, compact the feature planes
 * to X[valid] in raster order (exactly the matrix scikit-learn sees), run rsseg_kmeans_fit_predict / rsseg_kmeans_predict /
 * rsseg_forest_predict* on the compacted planes unchanged, expand the per-pixel results back with a fill value.
 * A mask is a uint8 plane; any non-zero byte means valid.  Planes, masks and outputs may have any alignment that holds their
 * element (16-byte accesses are used where 16-byte alignment holds).  n < 2^39.  Errors name the argument. */
#define RSSEG_VALID_NAN 1     /* a NaN in any plane makes the pixel invalid */
#define RSSEG_VALID_INF 2     /* +-inf in any plane */
#define RSSEG_VALID_VALUE 4   /* a value equal to `nodata` cast to the planes' type (a value the type cannot hold matches nothing) */
/* d_mask[i] = 1 iff pixel i passes every test of `flags` in every one of the P planes (dtype RSSEG_F32, RSSEG_F64 or RSSEG_U8;
 * P <= 64) and, when d_and is given, d_and[i] != 0; else 0.  One pass over the planes.  *n_valid = the number of ones
 * (integer atomics, one per workgroup).  n == 0 is legal.  Synchronous.  Profiler name "valid_mask". */
int rsseg_valid_mask(rsseg_ctx *ctx, const void *const *d_planes, int P, int dtype, int64_t n, int flags, double nodata,
                     const uint8_t *d_and /* NULL or uint8[n] */, uint8_t *d_mask, int64_t *n_valid);
/* host-only: pixels per tile, and tiles one workgroup of the scan step takes per pass (tests place their seams by them) */
int rsseg_compact_tile(void);
int rsseg_compact_scan_span(void);
/* The plan of a mask: d_tile_off[t] = the number of valid pixels before tile t, for t = 0 .. ceil(n / tile); the last entry
 * and *n_valid are the mask's valid count.  Two launches (per-tile count, then one workgroup's scan over the counts), no
 * workgroup waits for another.  d_tile_off is the CALLER's device buffer of ceil(n / tile) + 1 int64: it must outlive the
 * classifier call that runs between compaction and expansion, and that call uses the context's workspace.  n == 0 is legal
 * (one entry, 0).  Synchronous.  Profiler name "compact_plan". */
int rsseg_compact_plan(rsseg_ctx *ctx, const uint8_t *d_mask, int64_t n, int64_t *d_tile_off, int64_t *n_valid);
/* d_out[p][rank(i)] = d_in[p][i] for every valid i, in raster order (rank(i) = valid pixels before i); P planes of elements
 * of elem_bytes (1, 4 or 8: any type of that size) in ONE launch, the mask bytes and in-tile ranks computed once per tile.
 * d_out[p] holds n_valid elements and overlaps no input plane.  With every pixel valid the result is a plain copy; with none
 * nothing is written.  Algorithmic HBM traffic: n mask bytes + per plane the 16-byte vectors of the input that hold a valid
 * pixel in, n_valid * elem_bytes out.  Profiler name "compact". */
int rsseg_compact_planes(rsseg_ctx *ctx, const uint8_t *d_mask, const int64_t *d_tile_off, int64_t n, const void *const *d_in, int P,
                         int elem_bytes /* 1, 4, 8 */, void *const *d_out);
/* d_out[i] = mask[i] ? d_in[rank(i)] : *fill, for i < n.  fill: host, elem_bytes.  d_in holds n_valid elements (NULL when
 * there are none); d_out must not overlap it (RSSEG_ERR_INVALID "d_out aliases d_in").  Profiler name "expand". */
int rsseg_expand_plane(rsseg_ctx *ctx, const uint8_t *d_mask, const int64_t *d_tile_off, int64_t n, const void *d_in, int elem_bytes,
                       const void *fill /* host, elem_bytes */, void *d_out);

/* ---- K22: Gaussian maximum-likelihood / Mahalanobis / minimum-distance classification ------------ */
/* One per-pixel sweep over F feature planes (RSSEG_F32 or RSSEG_F64, band-planar) for a model of k classes, all host arrays:
 * mean[k][F]; whiten[k][F (F + 1) / 2], the rows of a lower-triangular W_j packed row-major; offset[k]; class_values[k],
 * distinct and 1..255 (0 is the label of an unclassified pixel); max_dist2 (+inf: no threshold).
 * Per pixel, in float64, j ascending: x_f = the plane value (a NaN reads as 0); d_f = x_f - mean[j][f]; z_i = the fma chain
 * over f = 0..i of W_j[i][f] * d_f from +0; m_j = the fma chain over i of z_i * z_i from +0; g_j = m_j + offset[j]; the
 * strictly smallest g_j wins (ties to the lowest j, a NaN g_j never wins) and the second smallest is the runner-up.
 *   d_labels  class_values[winner], or 0 when no class won or m_winner > max_dist2
 *   d_dist2   NULL or float32(m_winner), NaN when no class won (written whether or not the threshold zeroed the label)
 *   d_margin  NULL or float32(second - best), NaN when no class won, +inf when k == 1
 * The kernel equals tests/gaussian_ref.py bit for bit.  Limits: 1 <= F <= 64 and 1 <= k <= 64, beyond them
 * RSSEG_ERR_UNSUPPORTED.  RSSEG_ERR_INVALID, naming the argument: a null or misaligned plane or output, a non-finite mean,
 * whiten or offset, a class value of 0 or one that occurs twice, a NaN max_dist2.  n == 0 returns RSSEG_OK and touches
 * nothing.  Planes and outputs may have any alignment that holds their element (16-byte loads where every plane is 16-byte
 * aligned and F <= 32).  Synchronous.  Profiler name "gauss_classify". */
int rsseg_gauss_classify(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype /* RSSEG_F32 | RSSEG_F64 */, int64_t n, int k,
                         const double *mean, const double *whiten, const double *offset, /* host */
                         const uint8_t *class_values, double max_dist2,
                         uint8_t *d_labels, float *d_dist2 /* or NULL */, float *d_margin /* or NULL */);

/* ---- K28: support vector machine classification (one-vs-one, libsvm's decision rule) ----------- */
#define RSSEG_SVM_RBF 0
#define RSSEG_SVM_POLY 1
#define RSSEG_SVM_LINEAR 2
#define RSSEG_SVM_MAX_CLASSES 16
#define RSSEG_SVM_MAX_SV 16384
#define RSSEG_SVM_MAX_DEGREE 8
/* One per-pixel sweep over F feature planes (RSSEG_F32 or RSSEG_F64, band-planar) for a model of k classes and S support
 * vectors, all host arrays, float64 unless said otherwise: offset[F] and scale[F] (finite, scale != 0); sv[S][F], the support
 * vectors in scaled units, grouped by class with the classes ascending (scikit-learn's order); n_support[k] (int, each >= 1,
 * summing to S); coef[k - 1][S] (scikit-learn's _dual_coef_); bias[P], P = k (k - 1) / 2, libsvm's -rho (scikit-learn's
 * _intercept_); class_values[k], distinct and 1..255; kernel, gamma, coef0, degree; w[P][F], the folded weights of the LINEAR
 * kernel (NULL otherwise).
 * Per pixel, in float64, every line one IEEE operation:
 *   x_f = the plane value widened, a NaN read as 0; a pixel with any +-inf x_f gets label 0 and margin NaN
 *   z_f = (x_f - offset_f) * scale_f
 *   RBF, per support vector i:   q = +0; f ascending: d = z_f - sv_if, q = fma(d, d, q);  K_i = svm_exp(-(gamma * q))
 *   POLY:   t = +0; f ascending: t = fma(sv_if, z_f, t);  u = fma(gamma, t, coef0);  K_i = u, then degree - 1 times K_i = K_i * u
 *   pairs p = (a, b), a < b, in the order (0,1), (0,2), ..., (k-2,k-1):  s = +0; over class a's support vectors ascending
 *   s = fma(coef[b-1][i], K_i, s), then over class b's s = fma(coef[a][i], K_i, s);  d_p = s + bias_p.  No term is skipped.
 *   LINEAR: d_p = (t = +0; f ascending: t = fma(w_pf, z_f, t)) + bias_p
 *   d_p > 0 is a vote for a, anything else (a NaN too) for b; the label is the lowest class index with the most votes
 *   margin = float32(the smallest |d_p| over the pairs that hold the winner); a NaN |d_p| is never the smallest (all NaN: +inf)
 * svm_exp(t), t <= 0:  t < -708 gives +0.  n = rint(t * LOG2E);  r = fma(-n, LN2_HI, t);  r = fma(-n, LN2_LO, r);  p = c_13,
 *   then j = 12 ... 0: p = fma(p, r, c_j), c_j the double nearest 1 / j!;  the result is p * 2^n, 2^n built from its exponent
 *   field (normal for every admitted t).  LOG2E = 0x3FF71547652B82FE, LN2_HI = 0x3FE62E42FEE00000, LN2_LO = 0x3DEA39EF35793C76.
 *   d_labels  class_values[winner], 0 for a pixel with an infinite plane value
 *   d_margin  NULL or float32
 * The kernel equals tests/svm_ref.py bit for bit.  Limits: 1 <= F <= 64, 2 <= k <= 16, 1 <= S <= 16384, 1 <= degree <= 8; beyond
 * them, or a kernel that is none of the three, RSSEG_ERR_UNSUPPORTED.  RSSEG_ERR_INVALID, naming the argument: k < 2, S < 1,
 * degree < 1, a null or misaligned plane or output, a missing model array, a non-finite model value, a scale of 0, an
 * n_support below 1 or not summing to S, a class value of 0 or one that occurs twice, an RBF gamma that is not > 0.
 * n == 0 returns RSSEG_OK and touches nothing.  Planes and outputs may have any alignment that holds their element.
 * Synchronous.  Profiler name "svm_classify". */
int rsseg_svm_classify(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype /* RSSEG_F32 | RSSEG_F64 */, int64_t n, int k, int S,
                       const double *offset, const double *scale, const double *sv, const int *n_support, const double *coef,
                       const double *bias, const uint8_t *class_values, int kernel /* RSSEG_SVM_* */, double gamma, double coef0, int degree,
                       const double *w /* LINEAR, else NULL */, uint8_t *d_labels, float *d_margin /* or NULL */);
/* The LINEAR kernel's folded weights w[P][F] (host, no context): for the pair p = (a, b) and the feature f the fma chain from
 * +0 of coef[b-1][i] * sv[i][f] over class a's support vectors ascending, then of coef[a][i] * sv[i][f] over class b's.
 * RSSEG_ERR_INVALID for a null array, F < 1, k < 2, S < 1 or an n_support that does not sum to S; k > 16 RSSEG_ERR_UNSUPPORTED. */
int rsseg_host_svm_fold_linear(int F, int k, int S, const double *sv, const int *n_support, const double *coef, double *w);

/* ---- K30: neural-network (multi-layer perceptron) classification --------------------------------- */
#define RSSEG_MLP_RELU 0
#define RSSEG_MLP_IDENTITY 1
#define RSSEG_MLP_LOGISTIC 2
#define RSSEG_MLP_TANH 3
#define RSSEG_MLP_MAX_HIDDEN_LAYERS 3
#define RSSEG_MLP_MAX_WIDTH 128
#define RSSEG_MLP_MAX_CLASSES 32
/* One pass over F feature planes (RSSEG_F32, band-planar, any element alignment) for a fitted scikit-learn MLPClassifier of k
 * classes, all host arrays, float32: widths[n_layers + 1] with widths[0] = F, widths[1 .. n_layers - 1] the hidden widths and
 * widths[n_layers] the output units, k for k >= 3 and 1 for k = 2 (scikit-learn's binary layout); weights, the concatenation
 * of W_l[widths[l-1]][widths[l]], l = 1 .. n_layers, row-major (coefs_); biases, the concatenation of b_l[widths[l]]
 * (intercepts_); offset[F] and scale[F] (finite, scale != 0); activation, RSSEG_MLP_*, of the hidden layers; class_values[k],
 * distinct and 1..255.
 * Per pixel, in float32 unless said otherwise, every line one IEEE operation:
 *   x_f = the plane value, a NaN read as +0; a pixel with any +-inf x_f gets label 0 and margin, confidence, probabilities NaN
 *   z_f = (x_f - offset_f) * scale_f;  h_0 = z
 *   layer l, unit j:  a = b_l[j]; i ascending: a = fmaf(h_(l-1)[i], W_l[i][j], a).  The chain starts at the bias; no term is
 *   skipped.  h_l[j] = activation(a) on the hidden layers:
 *     relu      a > 0 ? a : +0 (a NaN gives +0);   identity  a
 *     logistic  in float64 on the widened a: e = svm_exp(-|a|); d = 1 + e; a >= 0 ? 1 / d : e / d; rounded once to float32
 *     tanh      |a| < 2^-13: a itself.  Otherwise in float64: e = svm_exp(-(2 |a|)); t = (1 - e) / (1 + e); a < 0 ? -t : t;
 *               rounded once to float32.  A NaN passes through both.  svm_exp is K28's (above), operation for operation.
 *   o_j = the last layer's a; for k = 2 the two logits are (+0, o_0)
 *   winner: w = 0, then j = 1 .. k-1 ascending: j replaces w when o_j > o_w, or when o_w is a NaN and o_j is not (the lowest j
 *   with the largest o_j; a NaN never beats anything; all NaN: j = 0).  second: the same rule over the logits without the winner.
 *   d_labels  class_values[winner]
 *   d_margin  NULL or float32: o_win - o_second, one float32 subtraction (|o_0| for k = 2)
 *   in float64: d_j = double(o_j) - double(o_win);  s = +0; j ascending: s = s + svm_exp(d_j)
 *   d_conf    NULL or float32(1 / s)
 *   d_proba   NULL or k float32 planes of n, plane j at d_proba + j * n: float32(svm_exp(d_j) / s)
 * Outputs are compared with tests/mlp_ref.py as values: -0 equals +0 and the NaN positions coincide (the kernel pads every chain
 * to a multiple of 4 terms with zeros, which can change nothing but the sign of a zero).
 * Limits: 1 <= F <= 64; 1 to 3 hidden layers (n_layers 2 .. 4), each 1 .. 128 wide; 2 <= k <= 32; the staged model must fit
 * LDS beside one tile of pixels (rsseg_mlp_plan).  Beyond them, or an unknown activation: RSSEG_ERR_UNSUPPORTED.
 * RSSEG_ERR_INVALID, naming the argument: a null or misaligned plane or output, a missing or non-finite model value, a scale of
 * 0, a width below 1, widths[0] != F, output units that are not k's, k < 2, a class value of 0 or one that occurs twice, n < 0.
 * n == 0 returns RSSEG_OK and touches nothing.  Synchronous.  Profiler name "mlp_classify". */
int rsseg_mlp_classify(rsseg_ctx *ctx, const void *const *d_planes, int F, int64_t n, int n_layers, const int *widths, const float *weights,
                       const float *biases, const float *offset, const float *scale, int activation /* RSSEG_MLP_* */, int k,
                       const uint8_t *class_values, uint8_t *d_labels, float *d_margin /* or NULL */, float *d_conf /* or NULL */,
                       float *d_proba /* or NULL: k float32 planes */);
/* Host only, no context: *fits = 1 when rsseg_mlp_classify takes a model of these widths (0: beyond the limits, or it does not
 * fit LDS), *tile_pixels = the pixels a workgroup takes at a time (0 when it does not fit).  Either pointer may be NULL. */
void rsseg_mlp_plan(int F, int n_layers, const int *widths, int k, int *fits, int *tile_pixels);

/* ---- K11: random-forest inference ---------------------------------------------------------- */
/* Flattened sklearn forest (tree_ arrays concatenated; children are tree-local, -1 = leaf).
 * value: (n_nodes_total x n_classes) float64 class fractions.  The forest is copied to the device
 * and stays loaded in the context until the next load or destroy. */
int rsseg_forest_load(rsseg_ctx *ctx, int n_trees, const int64_t *tree_off, const int32_t *left,
                      const int32_t *right, const int32_t *feature, const double *threshold,
                      const uint8_t *missing_go_left, const double *value, int n_classes,
                      const int64_t *classes, int n_features);
/* predict_image (modules/supervised_classifiers.py:99-115) / supervised_classification_predict
 * (modules/features/extract.py:690-719): d_planes[F] float32 feature planes -> int64 class per pixel. */
int rsseg_forest_predict(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, int64_t *d_out);
/* RandomForestClassifier.predict_proba of the loaded forest (sklearn/ensemble/_forest.py:908-946), bit for bit: the leaf
 * rows of the trees added in tree order in float64, divided by the tree count.  One launch fills what is asked for:
 *   d_proba   [n_classes][n] float64, class-planar (class c of pixel i at c * n + i; the forest's own classes, no padding)
 *   d_conf    [n] float64, the largest class probability of the pixel
 *   d_labels  [n] int64, exactly what rsseg_forest_predict writes (first maximum on ties)
 * Any of the three may be null, not all three.  Errors are status codes (RSSEG_ERR_INVALID: no forest loaded, F is not the
 * forest's feature count, a null plane, every output null); n == 0 returns RSSEG_OK and touches nothing.
 * Profiler name "forest_proba". */
int rsseg_forest_predict_proba(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, double *d_proba, double *d_conf,
                               int64_t *d_labels);
/* The out-of-bag sums of the loaded forest over its own training samples (ForestClassifier._compute_oob_predictions,
 * _forest.py:558-622).  d_counts: [n_trees][n] int32 bootstrap counts, the layout rsseg_forest_fit takes; tree t votes for
 * sample i only where d_counts[t * n + i] == 0.  d_oob: [n_classes][n] float64, the sum of those trees' leaf rows in tree
 * order divided by max(number of such trees, 1); d_n_oob: [n] int32, that number (0: no tree left the sample out, the
 * row of d_oob is all zero).  RSSEG_ERR_INVALID as above, and for null counts or a null output; n == 0 returns RSSEG_OK.
 * Profiler name "forest_oob". */
int rsseg_forest_oob(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_counts, double *d_oob,
                     int32_t *d_n_oob);
/* The counts behind sklearn.inspection.permutation_importance (inspection/_permutation_importance.py:43-85) of the loaded
 * forest with accuracy as the score: for every job j = (feature f, source row s)
 *   counts[j] = #{ i < n : label_index(x_i with x_i[f] := d_planes[f][d_src[s * n + i]]) == d_y[i] }
 * label_index: the class index rsseg_forest_predict turns into classes[...] (float64 sums in tree order, first maximum on
 * ties); feature -1 substitutes nothing (the baseline score) and ignores `source`.
 * d_y: [n] int32 class indices, -1 for a label the forest does not know (never correct); d_src: [n_src][n] int32 rows of
 * sample indices, each in [0, n) (an index outside is not dereferenced: RSSEG_ERR_INVALID "source index out of range");
 * jobs[n_jobs], counts[n_jobs]: host arrays.  Every job of the call runs in one launch (jobs on the grid's second axis;
 * one launch per 65535 jobs), each workgroup adds its integer count with one 64-bit atomic, and the call waits once;
 * the counters are zeroed on the context's stream inside the call.  The NaN-aware walk is chosen per job from the values
 * after the substitution.  Synchronous.
 * RSSEG_ERR_INVALID: no forest loaded, F is not the forest's feature count, a null plane, null d_y / jobs / counts, d_src
 * null while a job has feature >= 0, a job's feature outside [-1, F), a job's source outside [0, n_src) while feature >= 0,
 * n >= 2^31; `counts` is then untouched.  n_jobs == 0 returns RSSEG_OK; n == 0 returns RSSEG_OK with zero counts.
 * Algorithmic HBM traffic per job: 4F + 12 B/sample in (planes, d_y, d_src, the gathered value), 8 B per workgroup out.
 * Profiler name "forest_perm". */
typedef struct rsseg_perm_job {
    int32_t feature;
    int32_t source;
} rsseg_perm_job;
int rsseg_forest_permutation_counts(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_y,
                                    const int32_t *d_src, int n_src, const rsseg_perm_job *jobs, int n_jobs, int64_t *counts);

/* ---- K16: random-forest training ------------------------------------------------------------ */
/* RandomForestClassifier(criterion='gini', splitter='best').fit of scikit-learn 1.7.2 on float32 features, tree for tree
 * and bit for bit: the depth-first builder (tree/_tree.pyx:141-333) with node_split_best (tree/_splitter.pyx:269-545), the
 * splitter's xorshift feature draws, the float32 FEATURE_THRESHOLD rules and the Gini proxy over integer class counts.
 * d_planes[F] (host array of device pointers): n float32 values each, the layout K11 reads; d_y: n class indices 0..C-1;
 * d_counts: int32 bootstrap counts, n per tree (tree t at t * n), or one row shared by every tree when same_counts != 0
 * (bootstrap=False: all ones).  Every count row is non-negative and sums to n: weighted_n_samples is taken as n (n bootstrap
 * draws, or n unit weights), and a row that does not is refused with RSSEG_ERR_INVALID ("do not sum to n") instead of growing
 * subtly different trees; seeds[n_trees]: each splitter's initial xorshift state (RandomState(seed).randint(0, 2^31-1));
 * max_depth (2^31-1 for None), min_samples_split, min_samples_leaf, max_features: resolved as tree/_classes.py:320-348 does.
 * node_off[n_trees+1] (host): node offsets with node_off[t+1] - node_off[t] = 2 m_t - 1, m_t = samples of tree t with a
 * non-zero count (the most nodes a tree can have).  Per node (device arrays of node_off[n_trees] records, tree-local ids in
 * sklearn's preorder): left / right child (-1 leaf), feature (-2 leaf), threshold (-2.0 leaf), impurity, n_node_samples,
 * the integer weighted_n_node_samples, missing_go_to_left, and value[node][C] = count_c / weighted_n_node_samples.
 * node_count[n_trees], max_depth_out[n_trees] (host): nodes built and deepest depth per tree.
 * Limits: F <= 64 and C <= 64 (else RSSEG_ERR_UNSUPPORTED), 1 <= n < 2^26 (every sum of squared counts stays exact in
 * double).  One workgroup per tree; each launch builds at most 2048 nodes per tree and the call issues continuation
 * launches (one host wait each) until every tree is done; a launch without progress, or more launches than the node
 * bound allows, is an error.  Synchronous.  Profiler name "forest_fit". */
int rsseg_forest_fit(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_y, int n_classes,
                     const int32_t *d_counts, int same_counts, int n_trees, const uint32_t *seeds, int max_depth,
                     int min_samples_split, int min_samples_leaf, int max_features, const int64_t *node_off,
                     int32_t *d_left, int32_t *d_right, int32_t *d_feature, double *d_threshold, double *d_impurity,
                     int32_t *d_n_node, int32_t *d_w_node, uint8_t *d_missing_left, double *d_value,
                     int64_t *node_count, int32_t *max_depth_out);
/* rsseg_forest_fit with one record per tree in place of the scalar parameters and same_counts: trees of different forests
 * (other depths, other leaf sizes, other training subsets) grow side by side in one call, one workgroup each, and the chain of
 * continuation launches is as long as the slowest tree needs.  rsseg_forest_fit itself is this call with uniform jobs
 * (counts_row = t or 0, weight_total = n).
 * d_counts: n_count_rows rows of n int32 counts; tree t reads row jobs[t].counts_row, and several trees may name one row.  A
 * row is non-negative and sums to the job's weight_total, the tree's weighted_n_samples (a mismatch is RSSEG_ERR_INVALID
 * naming the tree and the expected sum; 1 <= weight_total < 2^26 as n above).  A sample with count 0 is not part of the tree,
 * exactly as scikit-learn's splitter drops samples of weight zero: with the bootstrap counts of a cross-validation fold's
 * training subset scattered into rows of length n (zeros at the held-out samples, weight_total = the subset's size) the tree
 * equals the one RandomForestClassifier.fit(X[train], y[train]) grows, provided `train` is sorted.
 * jobs[n_trees] (host): seed, max_depth, min_samples_split, min_samples_leaf, max_features as rsseg_forest_fit takes them,
 * per tree; `reserved` is 0.  node_off, the node arrays, node_count and max_depth_out: as rsseg_forest_fit.
 * Profiler name "forest_fit_jobs". */
typedef struct rsseg_forest_job {
    int64_t counts_row;
    int64_t weight_total;
    uint32_t seed;
    int32_t max_depth, min_samples_split, min_samples_leaf, max_features;
    int32_t reserved;
} rsseg_forest_job;
int rsseg_forest_fit_jobs(rsseg_ctx *ctx, const float *const *d_planes, int F, int64_t n, const int32_t *d_y, int n_classes,
                          const int32_t *d_counts, int64_t n_count_rows, int n_trees, const rsseg_forest_job *jobs,
                          const int64_t *node_off, int32_t *d_left, int32_t *d_right, int32_t *d_feature, double *d_threshold,
                          double *d_impurity, int32_t *d_n_node, int32_t *d_w_node, uint8_t *d_missing_left, double *d_value,
                          int64_t *node_count, int32_t *max_depth_out);

/* ---- K12: rule-based classification --------------------------------------- */
/* threshold_segmentation (modules/features/extract.py:344-404, otsu=False): NaN counts as 0, then d_out = 1 where
 * lo < x < hi, else 0 (pass -INFINITY / INFINITY for `x > t` / `x < t`). */
int rsseg_threshold_band_f32(rsseg_ctx *ctx, const float *d_x, int64_t n, float lo, float hi, uint8_t *d_out);
/* The band conditions of extract_bareland_by_rule (extract.py:486-497: np.logical_and(x > lo, x < hi) on the raw plane):
 * nan_as_zero = 0 leaves a NaN pixel outside every interval (both comparisons are false); nan_as_zero = 1 is
 * rsseg_threshold_band_f32. */
int rsseg_band_interval_f32(rsseg_ctx *ctx, const float *d_x, int64_t n, float lo, float hi, int nan_as_zero, uint8_t *d_out);
/* The same on a float64 plane (the comparisons of a float64 feature with a Python-float threshold are float64 comparisons). */
int rsseg_band_interval_f64(rsseg_ctx *ctx, const double *d_x, int64_t n, double lo, double hi, int nan_as_zero, uint8_t *d_out);
/* threshold_segmentation(..., otsu=True) (extract.py:358-371): NaN -> 0; *vmin / *vmax = the plane's extrema; when they are
 * equal d_out is all 0 (above) / all 1 and *level = -1; otherwise the plane is stretched to uint8 in its own dtype
 * (np.clip((x - min) / (max - min + 1e-10) * 255, 0, 255).astype(uint8)), *level = cv2.threshold(THRESH_OTSU)'s level of its
 * 256-bin histogram (OpenCV's getThreshVal_Otsu_8u restated), and d_out = q > level (above) or its complement.
 * dtype: RSSEG_F32 or RSSEG_F64.  Whole raster on one GPU. */
int rsseg_otsu_mask(rsseg_ctx *ctx, const void *d_x, int dtype, int64_t n, int above, uint8_t *d_out, int *level, double *vmin,
                    double *vmax);
/* Mask algebra of extract_builtup_by_threshold / extract_bareland_by_rule (extract.py:447-505) on 0 / 1 planes:
 * op 0: a & b, 1: a | b, 2: a & !b, 3: !a (d_b may be NULL).  d_out may alias an input. */
int rsseg_mask_op_u8(rsseg_ctx *ctx, const uint8_t *d_a, const uint8_t *d_b, int64_t n, int op, uint8_t *d_out);
/* final_map[mask == 1] = value, or only where final_map == 0 (scripts/3_classification.py:361-363, 373). */
int rsseg_mask_paint_u8(rsseg_ctx *ctx, uint8_t *d_map, const uint8_t *d_mask, int64_t n, int value, int only_unset);
/* cv2.morphologyEx / erode / dilate with cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), k odd in 3 ... 31, on a uint8
 * plane (advanced_post_processing, extract.py:311-313, 334-336): op = RSSEG_MORPH_ERODE / DILATE / OPEN / CLOSE. */
int rsseg_morph_ellipse_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int k, int op, uint8_t *d_out);
/* scipy.ndimage.label(mask, structure=ones((3,3))) + the np.bincount area filter (extract.py:319-329): d_out = mask
 * without its 8-connected components of fewer than min_area pixels.  Whole raster on one GPU (components cross
 * stripes, so this operator is not row-sharded). */
int rsseg_remove_small_components_u8(rsseg_ctx *ctx, const uint8_t *d_mask, int H, int W, int min_area, uint8_t *d_out);
/* scipy.ndimage.binary_fill_holes(mask) (advanced_post_processing's branch for an even or zero smooth_kernel_size,
 * extract.py:314-316): d_out = mask plus every 4-connected background component that touches no image border.
 * Whole raster on one GPU. */
int rsseg_fill_holes_u8(rsseg_ctx *ctx, const uint8_t *d_mask, int H, int W, uint8_t *d_out);

/* ---- K20: clean-up of a class map (no counterpart in the reference) --------------------------- */
/* A class map is a uint8 plane; every result below is an integer, so the kernels are exact by construction.
 * counts (host, 256): how often every byte value occurs among the n bytes of d_q.  Profiler name "class_hist". */
int rsseg_hist_u8(rsseg_ctx *ctx, const uint8_t *d_q, int64_t n, int64_t *counts);
/* d_q[i] = to wherever d_q[i] == from, in place; n_replaced (may be NULL): how many.  from, to in 0 ... 255. */
int rsseg_replace_u8(rsseg_ctx *ctx, uint8_t *d_q, int64_t n, int from, int to, int64_t *n_replaced);
/* k x k majority (mode) filter, k odd in 3 ... 15.  The window is centred on the pixel and clipped to the image: cells
 * outside do not vote.  ignore / fill: a value 0 ... 255 or -1 for none (equal values are refused).  `ignore` pixels never
 * vote and are never changed; `fill` pixels never vote and take their window's winner when the window has a voter, else
 * stay; with fill_only != 0 every pixel that is not `fill` keeps its value.  Winner: the label with the most votes; on a tie
 * the centre's own label if it votes and is among the maxima, otherwise the smallest tied label.
 * Rows form: d_q holds Hin rows, which are rows [img_y0, img_y0 + Hin) of an image of img_H rows; rows [y0, y1) of the
 * plane are produced into the compact (y1 - y0) x W plane d_out (not d_q).  The window is clipped against the image's first
 * and last row, so every image row it reaches must be in the plane (R = k / 2 halo rows on a side that is not an image
 * edge), and a stripe gets exactly the rows of the un-sharded result.  The whole map: y0 = img_y0 = 0, y1 = Hin = img_H.
 * group_mask: bit g set when a label in 8g ... 8g + 7 may occur (a superset is exact, only slower; the output's labels are
 * among the input's, so one mask serves repeated passes); 0: taken from a histogram of the plane inside the call.
 * n_changed: produced pixels whose output differs from their input; n_unfilled: produced `fill` pixels still `fill`.
 * RSSEG_ERR_INVALID, naming the argument: null pointers, d_out == d_q, k, ignore, fill, rows outside the plane, a plane
 * outside the image, a missing halo.  Synchronous (the counters are on the host).  Profiler name "majority". */
int rsseg_majority_u8(rsseg_ctx *ctx, const uint8_t *d_q, int Hin, int W, int y0, int y1, int img_y0, int img_H, int k, int ignore, int fill,
                      int fill_only, uint32_t group_mask, uint8_t *d_out, int64_t *n_changed, int64_t *n_unfilled);
/* Multi-class sieve: pixels are connected when they are 8-neighbours (connectivity 8) or 4-neighbours (4), hold the same
 * label and that label is not `ignore` (0 ... 255, or -1 for none); every component of fewer than min_area pixels is written
 * as removed_value (0 ... 255), everything else is copied; min_area <= 1 is the identity.  n_removed: the pixels of the
 * removed components.  One labelling pass for any number of classes (the union-find of rsseg_remove_small_components_u8).
 * Whole raster on one GPU; H * W <= 2^31 - 1, else RSSEG_ERR_UNSUPPORTED.  RSSEG_ERR_INVALID, naming the argument: null
 * pointers, d_out == d_q, connectivity, ignore, removed_value.  Synchronous.  Profiler name "sieve". */
int rsseg_sieve_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int min_area, int connectivity, int ignore, int removed_value,
                   uint8_t *d_out, int64_t *n_removed);

/* ---- K23: SLIC superpixels and object-based class maps (no counterpart in the reference) -------- */
/* Superpixels of P (1 ... 16) uint8 planes of H x W pixels; d_mask: NULL (all valid) or H * W bytes, 0 = not valid.  Every
 * result has one right answer, restated in tests/slic_ref.py, and the kernels give it bit for bit.
 * Grid: ny = ceil(H / S), nx = ceil(W / S) centres, id k = cy * nx + cx; the cell of a pixel is (y / S, x / S) and its
 * first label is its cell's id.  Centre k: count, sum y, sum x, sum q_p over the valid pixels labelled k (integers), each
 * mean float64(sum) / float64(count); a centre without a pixel is dead.  Iteration t = 1 ... max_iter: every valid pixel takes,
 * among the live centres of the 3 x 3 cells around its cell, visited in ascending id, the first with a strictly smaller
 *   D = dc + weight * ds,  dc = sum_p (q_p - c_p)^2 (p ascending, from 0.0),  ds = (y - c_y)^2 + (x - c_x)^2
 * (float64, every multiply and add one IEEE operation); if no label changed the iterations stop with *n_iter = t, otherwise
 * the centres are recomputed; *n_iter = max_iter when they never stop, and max_iter = 0 leaves the grid.
 * Connectivity (always): the 4-connected components of equal label; those of fewer than min_area pixels (none when
 * min_area <= 1) give up their pixels, which are regrown in rounds: every unassigned valid pixel takes the segment of the
 * first of its up, left, right, down neighbours that was assigned when the round began, until a round assigns none
 * (*n_regrown: pixels assigned this way).  What no round reaches keeps its small component as its segment.
 * d_labels (int32, H * W, 4-byte aligned): 0 for a masked pixel, else 1 ... *n_segments, numbered in the order of the
 * segments' smallest pixel index.  weight: finite, >= 0 ((m / S)^2 for compactness m); 2 <= S <= 4096; max_iter, min_area >= 0
 * (RSSEG_ERR_INVALID, naming the argument); P > 16 or H * W > 2^31 - 1: RSSEG_ERR_UNSUPPORTED.  Whole raster on one GPU.
 * Synchronous.  Profiler names "slic_init", "slic_assign", "slic_enforce", "slic_relabel". */
int rsseg_slic_u8(rsseg_ctx *ctx, const uint8_t *const *d_planes, int P, int H, int W, const uint8_t *d_mask, int S, double weight, int max_iter,
                  int min_area, int32_t *d_labels, int64_t *n_segments, int *n_iter, int64_t *n_regrown);
/* host-only: the tile of the assignment kernel (columns, rows), for the tests that straddle its seams */
void rsseg_slic_tile(int *tile_w, int *tile_h);
/* The reductions below take a segment plane d_seg (int32) with labels 0 ... n_segments, 0 meaning "no segment"; a label
 * outside that range is RSSEG_ERR_INVALID (it is never used as an index).
 * d_sums (device, int64[(n_segments + 1)][3 + P], row 0 all zero): per segment the pixel count, sum y, sum x and the sum of
 * each of the P (0 ... 16) planes, over the pixels whose d_mask byte (NULL: all) is non-zero.  dtype RSSEG_U8: the bytes;
 * RSSEG_F32: llrint(x * 2^40) (round to nearest even), exact for |x| < 2^11; the caller keeps count * max|x| below 2^23 and
 * NaN out.  Integer sums: the result does not depend on the order of the atomics.  Profiler name "segment_sums". */
int rsseg_segment_sums(rsseg_ctx *ctx, const int32_t *d_seg, int H, int W, int64_t n_segments, const void *const *d_planes, int P, int dtype,
                       const uint8_t *d_mask, int64_t *d_sums);
/* d_table (device, uint8[n_segments + 1]): per segment the label of d_class (uint8, n pixels) with the most votes among its
 * pixels, ties to the smallest label; `ignore` (0 ... 255, -1: none) never votes; a segment without a voter, and entry 0,
 * get `fill` (0 ... 255).  The vote table is n_segments x (largest voting label + 1) int32: above 2 GiB is
 * RSSEG_ERR_UNSUPPORTED.  Profiler name "segment_majority". */
int rsseg_segment_majority_u8(rsseg_ctx *ctx, const int32_t *d_seg, int64_t n, int64_t n_segments, const uint8_t *d_class, int ignore, int fill,
                              uint8_t *d_table);
/* d_out[i] = d_table[d_seg[i]]; elements of elem_bytes = 1 or 4 (uint8, float32, int32); entry 0 is the caller's.
 * Profiler name "segment_paint". */
int rsseg_segment_paint(rsseg_ctx *ctx, const int32_t *d_seg, int64_t n, int64_t n_segments, const void *d_table, int elem_bytes, void *d_out);

/* ---- K25: the object table: what describes a segment (no counterpart in the reference) -------- */
#define RSSEG_OBJ_GEOMETRY 1
/* d_table (device, int64[(n_segments + 1)][11 + 4 P], 8-byte aligned).  A pixel i is COUNTED for segment s when d_seg[i] == s,
 * s >= 1 and its d_mask byte (NULL: all) is non-zero; its effective label is s, every other pixel's is 0.
 * Columns: 0 n; 1, 2 sum y, sum x; 3, 4, 5 sum y^2, sum x^2, sum y x; 6 ... 9 min y, max y, min x, max x; 10 the perimeter:
 * the number of (counted pixel, side) pairs whose neighbour across that side lies outside the image or has another
 * effective label (label 0 and masked pixels included, so holes count).  Plane p: columns 11 + 4 p ... 11 + 4 p + 3 = sum q,
 * sum q2, min q, max q.  RSSEG_U8: q = v, q2 = v v.  RSSEG_F32: q = llrint(v 2^40) (the column of rsseg_segment_sums),
 * q2 = llrint((double)v (double)v 2^24): the product is exact in float64 and never a tie, one rounding per term.  The caller
 * keeps float planes free of NaN, |v| < 2^11 and count * max|v| < 2^23 over the counted pixels, as for rsseg_segment_sums.
 * A row without a counted pixel (row 0 always) holds 0 in the sums, min y = H, max y = -1, min x = W, max x = -1,
 * min q = INT64_MAX, max q = INT64_MIN.  Without RSSEG_OBJ_GEOMETRY in flags columns 1 ... 10 hold these empty values in
 * every row (the neighbours are not read); column 0 is always filled.  Integer sums, minima and maxima: one right answer,
 * restated in tests/objects_ref.py.
 * RSSEG_ERR_INVALID, naming the argument, before any launch: a null or misaligned pointer, H or W < 1, H W > 2^31 - 1, P < 0,
 * a wrong dtype, unknown flag bits; and after the pass a label outside 0 ... n_segments (never used as an index).
 * RSSEG_ERR_UNSUPPORTED: P > 16, or H W max(H, W)^2 >= 2^63 (the coordinate moments would leave int64; 32768^2 is inside).
 * Whole raster on one GPU.  Synchronous.  Profiler name "segment_features". */
int rsseg_segment_features(rsseg_ctx *ctx, const int32_t *d_seg, int H, int W, int64_t n_segments, const void *const *d_planes, int P,
                           int dtype /* RSSEG_U8 | RSSEG_F32 */, const uint8_t *d_mask, int flags /* RSSEG_OBJ_GEOMETRY */, int64_t *d_table);
/* host-only: the kernel's tile and the rows of its per-tile table in LDS; a tile that meets more segments commits the surplus
 * straight to d_table (for tests that place segments across the seams and force that path) */
void rsseg_segment_features_plan(int P, int *tile_w, int *tile_h, int *lds_slots);

/* ---- K27: the region adjacency graph of a segment map (no counterpart in the reference) -------- */
/* d_edges (device, int64[max_edges][3 + P], 8-byte aligned): one row per unordered pair of segments that share a border.
 * The effective label of a pixel is K25's: d_seg[i] where it is 1 ... n_segments and the d_mask byte (NULL: all) is non-zero,
 * else 0.  A CROSSING is a pixel and its right or its lower neighbour (4-connectivity) whose effective labels a != b are both
 * > 0; every crossing belongs to its left / upper pixel and is counted once.
 * Columns: 0, 1 min(a, b), max(a, b); 2 the length: the number of crossings of the pair; 3 + p the contrast of uint8 plane p:
 * the sum over the crossings of |v_p(pixel) - v_p(neighbour)|.  0 <= P <= 16.  *n_edges: the number of rows written; their
 * ORDER IS UNSPECIFIED (Context.segment_adjacency sorts them).  Integer sums: one right answer, restated in
 * tests/adjacency_ref.py.
 * Capacity: the library builds its own open-addressing table in the context's workspace, max_edges + max_edges / 2 + 64 rows of
 * 2 + P int64.  The call returns RSSEG_ERR_UNSUPPORTED ("more than max_edges ... distinct pairs") exactly when the raster holds
 * more than max_edges distinct pairs, and succeeds with max_edges equal to their number; d_edges is then not to be read.
 * RSSEG_ERR_INVALID, naming the argument, before any launch: a null or misaligned pointer, H or W < 1, H W > 2^31 - 1, P < 0,
 * max_edges < 0; and after the pass a label outside 0 ... n_segments (never used as an index).  RSSEG_ERR_UNSUPPORTED: P > 16.
 * RSSEG_ERR_NOMEM: the table could not be allocated.
 * Whole raster on one GPU.  Synchronous.  Profiler names "segment_adjacency" (the pass) and "segment_adjacency_compact". */
int rsseg_segment_adjacency(rsseg_ctx *ctx, const int32_t *d_seg, int H, int W, int64_t n_segments, const uint8_t *d_mask,
                            const uint8_t *const *d_planes, int P, int64_t max_edges, int64_t *d_edges, int64_t *n_edges);
/* host-only: the kernel's tile and the rows of its per-tile table in LDS; a tile that meets more pairs commits the surplus
 * straight to the global table (for tests that place segments across the seams and force that path) */
void rsseg_segment_adjacency_plan(int P, int *tile_w, int *tile_h, int *lds_slots);

/* ---- K24: class signatures: per-label sums of 1, x and x x^T (no counterpart in the reference) -- */
/* d_out (device, int64[n_classes][1 + F + F (F + 1) / 2], 8-byte aligned): per label the exact integer moments of F
 * feature planes (RSSEG_F32 or RSSEG_U8, band-planar, n_local pixels) over the counted pixels.  One right answer, restated in
 * tests/moments_ref.py; the kernel gives it bit for bit whatever the workgroup count, tile or path.
 * Counted: the mask byte is non-zero (d_mask NULL: all) and the label (RSSEG_U8 or RSSEG_I32) differs from `ignore` (-1: no
 * label is ignored).  A counted label outside 0 ... n_classes - 1 is RSSEG_ERR_INVALID and is never used as an index.
 * RSSEG_F32: v_f = the plane value, a NaN read as +0; u_f = v_f * 2^plane_exp[f] (exact, in float64); a counted pixel with any
 * |u_f| > 1 (+-inf included) enters no column and is counted in *n_left_out.  Otherwise row `label` takes
 *   column 0                  += 1
 *   column 1 + f              += rint(u_f * 2^Q)
 *   column 1 + F + tri(a, b)  += rint(u_a * 2^Q * u_b)     a <= b, tri = the row-major index in the upper triangle
 * the product exact (two 24-bit significands) and rounded once, to nearest-even: fma(u_a * 2^Q, u_b, 1.5 * 2^52).
 * RSSEG_U8: the columns are the plain integers 1, v_f and v_a * v_b; plane_exp must be NULL and Q 0; *n_left_out = 0.
 * Limits: 1 <= F <= 64 and 1 <= n_classes <= 256 (above: RSSEG_ERR_UNSUPPORTED); 0 <= Q <= 50, n_local * 2^Q < 2^62,
 * |plane_exp[f]| <= 300; RSSEG_ERR_INVALID, naming the argument, for these, a null pointer or a plane, label plane or table
 * not aligned to its element.  n_local == 0 writes zeros.  Planes, labels and mask may have any alignment that holds their
 * element.  With a communication hook installed the table and *n_left_out are summed over the ranks (int64 SUM through the
 * communication buffer).  Synchronous.  Profiler name "class_moments". */
int rsseg_class_moments(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype /* RSSEG_F32 | RSSEG_U8 */, int64_t n_local,
                        const void *d_labels, int label_dtype /* RSSEG_U8 | RSSEG_I32 */, int n_classes, int ignore /* -1: none */,
                        const uint8_t *d_mask /* NULL or n_local bytes, 0 = not counted */,
                        const int *plane_exp /* host, F */, int Q,
                        int64_t *d_out /* device, int64[n_classes][1 + F + F (F + 1) / 2] */, int64_t *n_left_out /* host */);
/* host-only: *path = 0 when the workgroup keeps its table in LDS (Path A), 1 when it adds into the global table (Path B), -1
 * outside the limits; *tile_pixels = the pixels a workgroup stages at a time.  For the tests that straddle the seams. */
void rsseg_class_moments_plan(int F, int n_classes, int dtype, int *path, int *tile_pixels);

/* ---- K26: ISODATA: assign to the nearest centre and take the clusters' moments in one pass (no counterpart in the reference) -- */
/* One ISODATA iteration's pass over F feature planes (RSSEG_F32 or RSSEG_U8, band-planar, n_local pixels) and k centres.  One
 * right answer, restated in tests/isodata_ref.py; the kernel gives it bit for bit whatever the workgroup count, tile or path.
 * Counted: the mask byte is non-zero (d_mask NULL: all).
 * RSSEG_F32: v_f = the plane value, a NaN read as +0; u_f = v_f * 2^plane_exp[f] (exact, in float64); a counted pixel with any
 * |u_f| > 1 (+-inf included) is LEFT OUT and counted in *n_left_out.  RSSEG_U8: u_f = v_f; plane_exp must be NULL and Q 0;
 * no pixel is left out.
 * Per counted pixel that is not left out, in float64 and one IEEE operation per written operation (no fma):
 *   z_f = u_f * weight[f];
 *   for j = 0 .. k - 1:  d_j = +0.0;  for f = 0 .. F - 1:  t = z_f - centers[j * F + f];  d_j = d_j + t * t;
 *   label = the lowest j with the strictly smallest d_j (j = 0 when no d_j is smaller than d_0);
 *   *n_changed += (label != the byte that was in d_labels);  d_labels = label;
 *   row `label` of d_table takes
 *     column 0          += 1
 *     column 1 + f      += rint(u_f * 2^Q)
 *     column 1 + F + f  += rint((u_f * 2^Q) * u_f)
 *   the product exact (two 24-bit significands) and rounded once, to nearest-even: K24's columns (0, 0), (0, 1 + f), (1 + f, 1 + f).
 * Every other pixel gets label 255, enters no column and is not counted in *n_changed.
 * d_table NULL: labels, *n_changed and *n_left_out only (the accumulation is not compiled into that kernel).
 * Limits: 1 <= F <= RSSEG_MAX_FEATURES and 1 <= k <= RSSEG_MAX_CLUSTERS (above: RSSEG_ERR_UNSUPPORTED); 0 <= Q <= 50,
 * n_local * 2^Q < 2^62, |plane_exp[f]| <= 300, every weight and centre finite; RSSEG_ERR_INVALID, naming the argument, for
 * these, a null pointer, a plane not aligned to its element or a table not 8-byte aligned.  n_local == 0 writes zeros.
 * Planes, labels and mask may have any alignment that holds their element.  The result is this context's own: a communication
 * hook, if installed, reduces nothing (the integers of the stripes of a sharded raster add).  Synchronous.  Profiler name
 * "isodata_sweep". */
int rsseg_isodata_sweep(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype /* RSSEG_F32 | RSSEG_U8 */, int64_t n_local,
                        const uint8_t *d_mask /* NULL or n_local bytes, 0 = not counted */,
                        const int *plane_exp /* host, F; NULL for RSSEG_U8 */, int Q,
                        const double *weight /* host, F */, int k, const double *centers /* host, k * F, in weighted units */,
                        uint8_t *d_labels /* device, n_local bytes, read and rewritten in place */,
                        int64_t *d_table /* device int64[k][1 + 2 F], or NULL: labels only */,
                        int64_t *n_changed, int64_t *n_left_out /* host */);
/* host-only: *path = 0 when the workgroup keeps its table in LDS (Path A), 1 when it adds into the global table (Path B), -1
 * outside the limits; *tile_pixels = the pixels a workgroup takes at a time.  For the tests that straddle the seams. */
void rsseg_isodata_plan(int F, int k, int dtype, int *path, int *tile_pixels);

/* ---- K29: Gaussian mixture: the E-step and the weighted moments of one EM iteration in one pass (no counterpart in the reference) -- */
/* One pass over F feature planes (RSSEG_F32 or RSSEG_U8, band-planar, n_local pixels) and a mixture of k components.  One right
 * answer, restated in tests/gmm_ref.py; the kernel gives it bit for bit whatever the workgroup count, tile or path.
 * Counted: the mask byte is non-zero (d_mask NULL: all).
 * RSSEG_F32: v_f = the plane value, a NaN read as +0; u_f = v_f * 2^plane_exp[f] (exact, in float64); a counted pixel with any
 * |u_f| > 1 (+-inf included) is LEFT OUT.  RSSEG_U8: u_f = v_f, plane_exp must be NULL, and the moments carry no fraction bits
 * (QM = 0 below; Q scales ll_sum alone).  RSSEG_F32: QM = Q.
 * The model is in u units, in K22's layout: mean[k][F], whiten[k][F (F + 1) / 2] the rows of the lower-triangular W_j packed
 * row-major, offset[k] = ln |S_j| - 2 ln w_j.
 * Per counted pixel that is not left out, in float64, one IEEE operation per written operation, fma only where written:
 *   1  g_j, j ascending, as rsseg_gauss_classify defines it with x_f = u_f:  d_f = u_f - mean[j][f];  z_i = the fma chain
 *      z = fma(W_j[i][f], d_f, z) over f = 0 .. i from +0;  m_j = the fma chain m = fma(z_i, z_i, m) over i from +0;
 *      g_j = m_j + offset[j].  diag != 0 evaluates z_i = fma(W_j[i][i], d_i, +0) alone (W_j is taken as diagonal).
 *   2  best = +inf, win = none;  g_j < best: best = g_j, win = j (the lowest j keeps a tie).  A pixel whose best is not finite is
 *      LEFT OUT.
 *   3  e_j = gmm_exp(-0.5 * (g_j - best)), gmm_exp = K28's svm_exp, operation for operation
 *   4  s = +0; j ascending: s = s + e_j
 *   5  r_j = e_j / s
 *   6  q_j = rint(r_j * 2^20)
 *   7  ll = fma(-0.5, best, gmm_log(s))
 * gmm_log(s), s in [1, 64]:  e = the exponent of s, m = its significand in [1, 2);  m > SQRT2 (0x3FF6A09E667F3BCD): m = m * 0.5,
 *   e = e + 1;  f = m - 1;  t = f / (2 + f);  z = t * t;  R = Lg7, i = 6 .. 1: R = fma(R, z, Lg_i);  R = R * z;
 *   hfsq = (0.5 * f) * f;  gmm_log = e * LN2_HI - ((hfsq - (t * (hfsq + R) + e * LN2_LO)) - f)
 *   with Lg1 .. Lg7 = 0x3FE5555555555593, 0x3FD999999997FA04, 0x3FD2492494229359, 0x3FCC71C51D8E78AF, 0x3FC7466496CB03DE,
 *   0x3FC39A09D078C69F, 0x3FC2F112DF3E5244 and K28's LN2_HI, LN2_LO.
 * Row j of d_table takes, for every pixel with q_j != 0 (a zero q_j adds nothing):
 *     column 0                   += q_j
 *     column 1 + f               += rint(q_j * u_f * 2^QM)
 *   diag == 0:  column 1 + F + tri(a, b)  += rint(q_j * u_a * u_b * 2^QM), a <= b, the row-major upper triangle (K24's columns)
 *   diag != 0:  column 1 + F + f          += rint(q_j * u_f * u_f * 2^QM)
 *   each term ONE rounding, to nearest-even, of the exact real product (q_j u_a 2^QM is exact in float64: 21 + 24 bits).
 * tail[0] = n_counted (the pixels that entered), tail[1] = n_left_out, tail[2] = n_far, the entered pixels with |ll| >= 2^20 or
 * ll NaN, which enter the moments but not tail[3] = ll_sum = the sum of rint(ll * 2^Q).
 * Per-pixel outputs, each optional (NULL): d_labels = win + 1, 0 where the pixel did not enter; d_posterior = float32(r_win);
 * d_loglik = float32(ll); d_proba: k planes of n_local float32, float32(r_j); NaN where the pixel did not enter.
 * d_table NULL: the accumulation is not compiled into that kernel (predict).
 * Limits: 1 <= F <= RSSEG_MAX_FEATURES, 1 <= k <= 32 (above: RSSEG_ERR_UNSUPPORTED); 0 <= Q <= 30 and n_local <= 2^(42 - Q), so
 * that no term passes 2^50 and no sum 2^62 (RSSEG_U8: also n_local <= 2^26); |plane_exp[f]| <= 300; the model finite;
 * RSSEG_ERR_INVALID, naming the argument, for these, a null pointer, a plane not aligned to its element or a table not 8-byte
 * aligned.  n_local == 0 writes zeros.  The result is this context's own (the integers of the stripes of a sharded raster add).
 * Synchronous.  Profiler name "gmm_sweep". */
int rsseg_gmm_sweep(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype /* RSSEG_F32 | RSSEG_U8 */, int64_t n_local,
                    const uint8_t *d_mask /* NULL or n_local bytes, 0 = not counted */,
                    const int *plane_exp /* host, F; NULL for RSSEG_U8 */, int Q, int k, int diag,
                    const double *mean, const double *whiten, const double *offset /* host */,
                    int64_t *d_table /* device int64[k][diag ? 1 + 2 F : 1 + F + F (F + 1) / 2], or NULL */,
                    uint8_t *d_labels, float *d_posterior, float *d_loglik, float *d_proba /* device, each may be NULL */,
                    int64_t *tail /* host, 4 */);
/* host-only: *path = 0 when the workgroup keeps its table in LDS (Path A), 1 when it adds into the global table (Path B), -1
 * outside the limits; *tile_pixels = the pixels a workgroup takes at a time. */
void rsseg_gmm_plan(int F, int k, int dtype, int diag, int *path, int *tile_pixels);

/* ---- K13: remaining texture members of the feature dictionary ---------------- */
/* calculate_lbp_features (indices.py:320-344): skimage.feature.local_binary_pattern(u8, n_points, radius, 'uniform');
 * d_out: the codes 0 .. n_points + 1 as uint8 (the caller divides by their maximum in float64, :342). */
int rsseg_lbp_uniform_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int n_points, double radius, uint8_t *d_out);
/* entropy_scale_k (indices.py:551-560): skimage.filters.rank.entropy(u8, disk(radius)), float64, radius in {1,2,3,5,7}
 * (the caller divides by the maximum, :559). */
int rsseg_rank_entropy_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int radius, double *d_out);
/* gaussian_5 / gaussian_15 (indices.py:463-464): cv2.GaussianBlur(u8, (ksize, ksize), 0), OpenCV's fixed-point path for
 * 8-bit images, BORDER_REFLECT_101; uint8 out (the caller divides by 255.0 and forms the DoG, :463-470). */
int rsseg_gaussian_blur_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int ksize, uint8_t *d_out);
/* host-only: the ksize taps of that blur in 8 fractional bits (they sum to 256). */
int rsseg_host_gaussian_kernel_fixed(int ksize, int *taps);

/* ---- K14: accuracy assessment -------------------------------------------------------------- */
/* The joint count table of (truth value, predicted value) over the pixels where truth > 0 (truth <= 0 is excluded, as
 * `valid_mask = roi_mask > 0` of scripts/4_evaluate.py:83 and `y_true > 0` of modules/evaluation.py:40 exclude it): the
 * np.unique / boolean-mask passes of ClassificationEvaluator.extract_valid_samples and map_clusters_to_classes
 * (scripts/4_evaluate.py:72-128) and the counting inside confusion_matrix, accuracy_score, cohen_kappa_score and
 * classification_report (:130-160, modules/evaluation.py:44-63).  Every one of those metrics follows exactly from the table.
 * d_truth: n_local labels of truth_dtype (RSSEG_U8, RSSEG_I16, RSSEG_U16, RSSEG_I32, RSSEG_I64); d_pred: n_local labels of
 * pred_dtype (RSSEG_U8, RSSEG_I32, RSSEG_I64); both 16-byte aligned.
 * known_range: NULL, or {tmin, tmax, pmin, pmax} the caller already knows to hold every valid pixel (KMeans labels 0..k-1,
 * a three-class map 0..3): the range pass is skipped; a valid pixel outside it is RSSEG_ERR_INVALID.  Otherwise one pass
 * finds the range: range_out = {tmin, tmax, pmin, pmax} of the valid pixels ({0, -1, 0, -1} and *n_valid = 0, no table,
 * when there is none).  counts (host, cap cells): the int64 table, row-major, cell (t - tmin) * np + (p - pmin) with
 * np = pmax - pmin + 1; *n_valid = the number of valid pixels.  A table of more than min(cap, 4096) cells is
 * RSSEG_ERR_UNSUPPORTED with range_out (and *n_valid, after a range pass) filled in.  Synchronous (results on the host).
 * With a communication path every rank's ranges go through the hook (RSSEG_I64 SUM of the count, MIN, MAX) and so does
 * the table (RSSEG_I64 SUM): each rank of a row-sharded map receives the whole raster's table, and every rank makes the
 * same hook calls, also when the table is over the cap. */
int rsseg_confusion_counts(rsseg_ctx *ctx, const void *d_truth, int truth_dtype, const void *d_pred, int pred_dtype, int64_t n_local,
                           const int64_t *known_range, int64_t range_out[4], int64_t *n_valid, int64_t *counts, int64_t cap);

/* ---- K15: preprocessing (stage 1) ----------------------------------------------------------- */
/* Radiometric calibration, the identity warp and the 8-bit min-max stretch of modules/features/preprocessing.py:54-125, as
 * scripts/1_preprocessing.py:25-85 chains them: per band b, radiance = gain[b] * DN + bias[b] in float64 (float32 for
 * float32 DN, the constants rounded to float32 first; two roundings, no fma), mn / mx = np.min / np.max of the radiance
 * (NaN when the band holds a NaN), then ((radiance - mn) * 255) / (mx - mn) in that dtype and .astype(np.uint8) as x86-64
 * NumPy casts it (truncation; 0 for NaN and +-inf, so a constant band, a band with a NaN and a band with an infinite
 * radiance range come out all zero).  Bit-exact.
 * d_in[n_bands]: n_local DN of in_dtype (RSSEG_U8, RSSEG_I16, RSSEG_U16, RSSEG_I32, RSSEG_F32, RSSEG_F64; anything else is
 * RSSEG_ERR_INVALID, named); d_out[n_bands]: n_local uint8; all 16-byte aligned; n_bands <= 16.
 * gain / bias: n_bands finite values, every gain > 0 (else RSSEG_ERR_INVALID); both NULL: the stretch alone, on values
 * already calibrated (image_enhancement of what it is handed; for int16 / int32 the caller keeps mx - mn within the type).
 * Two passes, both enqueued without a host wait: per band the min / max of the non-NaN DN and the NaN count (one partial per
 * workgroup, reduced on the device), then the stretch, whose workgroups derive the radiance range from that record (8-bit
 * DN through a 256-entry table in LDS).  With a communication path the record goes through the hook (RSSEG_F64 MIN and
 * MAX, RSSEG_I64 SUM of the NaN counts): every rank of a row-sharded raster is stretched with the whole raster's range.
 * range_out: NULL, or (host) double[n_bands][3] = {min, max of the non-NaN DN (+inf, -inf when there is none), NaN count}
 * of the whole raster, read back with the only host wait of the call.  Profiler names "pre_range", "pre_stretch". */
int rsseg_preprocess_u8(rsseg_ctx *ctx, const void *const *d_in, int in_dtype, int n_bands, int64_t n_local, const double *gain,
                        const double *bias, uint8_t *const *d_out, double *range_out);
/* radiometric_calibration of one band (preprocessing.py:54-74): d_out[i] = gain * d_in[i] + bias, float64 (RSSEG_F64
 * output), or float32 for RSSEG_F32 input (float32 constants and operations, as NumPy 2 promotes).  in_dtype as above;
 * gain and bias finite. */
int rsseg_radiometric(rsseg_ctx *ctx, const void *d_in, int in_dtype, int64_t n, double gain, double bias, void *d_out);

/* ---- K21: geometric correction (beyond the reference, whose geometric_correction warps with the identity) -------- */
#define RSSEG_WARP_NEAREST 0
#define RSSEG_WARP_BILINEAR 1
#define RSSEG_WARP_CUBIC 2   /* cubic convolution, Keys a = -0.5 */
/* Polynomial resampling of n_planes (1 ... 16) source planes of H x W pixels and one dtype (RSSEG_U8, RSSEG_I16, RSSEG_U16,
 * RSSEG_I32, RSSEG_F32, RSSEG_F64; anything else is RSSEG_ERR_INVALID, named) onto Ho x Wo planes of out_dtype (in_dtype,
 * RSSEG_F32 or RSSEG_F64).  coef = {p0..p5, q0..q5}; per output pixel (r, c), in double and one IEEE operation per written
 * operation:  X = (c + 0.5) - cx, Y = (r + 0.5) - cy,
 *   u = ((((p0 + p1*X) + p2*Y) + p3*(X*X)) + p4*(X*Y)) + p5*(Y*Y), v likewise from q: the source position in pixel-corner
 * coordinates (the first pixel's centre is (0.5, 0.5)).  The pixel is valid iff 0 <= u < W && 0 <= v < H (a NaN is not);
 * an invalid pixel gets `fill` and mask 0.  A valid one samples at fx = u - 0.5, fy = v - 0.5 with edge-replicated taps:
 * nearest (the tap floor(fy + 0.5), floor(fx + 0.5), bits preserved), bilinear (top = g00*(1-tx) + g01*tx, bot likewise,
 * top*(1-ty) + bot*ty) or cubic convolution (rows i = -1..2 summed ascending from 0.0, then columns), in double; integer
 * outputs are rint (half to even) and saturated, float32 is one cast.  tests/warp_ref.py restates it; results are bit-equal.
 * d_mask: NULL, or Ho * Wo uint8 (1 = sampled, 0 = fill); n_valid: NULL, or the number of valid pixels (the one host wait).
 * fill must be a value of an integer out_dtype (RSSEG_ERR_INVALID otherwise); coef, cx, cy finite; H, W, Ho, Wo >= 1 and
 * H * W, Ho * Wo < 2^39 (RSSEG_ERR_UNSUPPORTED).  Whole planes on one GPU: RSSEG_ERR_UNSUPPORTED on a context with a
 * communication path.  Planes aligned to their element.  Profiler name "warp". */
int rsseg_warp_poly(rsseg_ctx *ctx, const void *const *d_in, int in_dtype, int n_planes, int H, int W, const double *coef, double cx,
                    double cy, int method, double fill, void *const *d_out, int out_dtype, int Ho, int Wo, uint8_t *d_mask,
                    int64_t *n_valid);

/* ---- host-only helper (no GPU needed) ------------------------------------------------------- */
/* The random draws of k-means++ as the library makes them (numpy RandomState(seed): MT19937, random_sample,
 * RandomState.choice over n equal weights — sklearn/cluster/_kmeans.py:213-270): *center_id = index of the first
 * centre, uniforms[(k-1) * (2 + floor(ln k))] = the uniform(size=L) draws of the later rounds.  Used by the CPU test
 * suite to pin the generator against NumPy. */
int rsseg_host_kmeans_draws(uint32_t seed, int64_t n, int dtype, int k, int64_t *center_id, double *uniforms);
/* TIFF LZW (TIFF 6.0 section 13, as libtiff / GDAL write it: MSB-first codes of 9..12 bits, early change) for the GeoTIFF
 * outputs the reference writes with rasterio compress='lzw' (scripts/2_feature_extraction.py:239-258,
 * scripts/3_classification.py:509-538); called per strip / tile by rsseg/tiff.py.  Return the number of bytes produced,
 * or a negative value (-2: output buffer too small, -3: corrupt stream). */
int64_t rsseg_host_lzw_encode(const uint8_t *in, int64_t n, uint8_t *out, int64_t cap);
int64_t rsseg_host_lzw_decode(const uint8_t *in, int64_t n, uint8_t *out, int64_t cap);
/* The model step of the PCA entry points (K3) on its own: what they compute on the host between the Gram pass and the
 * projection.  limbs[2 * 44]: the exact sums over the N fitted pixels in quanta of 2^-Q, entry i as the pair
 * {limbs[2i], limbs[2i + 1]} with value (limbs[2i] << 32) + limbs[2i + 1]; entries 0..7 are the sums of x_b, entry
 * 8 + 8b - b(b-1)/2 + (c - b) is the sum of x_b * x_c for b <= c < 8 (entries of bands >= nb are not read).
 * Steps: sum * 2^-Q as a double; scikit-learn's float32 mean and covariance (g - (N * mu_b) * mu_c) / (N - 1); cyclic Jacobi
 * in float64; eigenvalues in stable descending order, clamped at 0; sign of each component by its first largest |entry|
 * (svd_flip); offs[c] = the float32 fma chain of mean_b * components[c][b]; ratios = variance / float32 running total.
 * Outputs (any may be NULL): mean[nb], cov[nb * nb], components[n_components * nb], explained_variance[n_components],
 * explained_variance_ratio[n_components], offs[n_components].  RSSEG_ERR_INVALID for nb outside 1..8, n_components
 * outside 1..nb or N < 2. */
int rsseg_host_pca_model(const int64_t *limbs, int64_t N, int Q, int nb, int n_components, float *mean, float *cov,
                         float *components, float *explained_variance, float *explained_variance_ratio, float *offs);

#ifdef __cplusplus
}
#endif
#endif /* RSSEG_H */
