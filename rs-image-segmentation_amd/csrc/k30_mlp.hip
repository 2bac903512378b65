// K30 — rsseg_mlp_classify: multi-layer perceptron (scikit-learn's MLPClassifier) classification of feature-planar float32
// rasters.  One pass; the arithmetic is the restatement's (tests/mlp_ref.py), operation for operation (include/rsseg.h has the
// contract): z_f = (x_f - offset_f) * scale_f, per layer and unit the float32 fma chain from the bias over the inputs ascending,
// the hidden activation, and on the last layer's sums the winner, the margin and the float64 softmax.
//
// The layers' products go through v_mfma_f32_16x16x4_f32: D = fma(a_k3, b_k3, fma(a_k2, b_k2, fma(a_k1, b_k1, fma(a_k0, b_k0,
// C)))), one rounding per product, so a k loop of them IS the contract's chain, with C started at the bias.  A is the weights
// (row = unit, lane l holds unit l & 15 at k = l >> 4), B the activations (column = pixel, lane l holds pixel l & 15 at
// k = l >> 4), D[unit 4 (l >> 4) + r][pixel l & 15] in register r.  K is padded to a multiple of 4 with zero weights AND zero
// activations (a zero times a NaN would not be neutral), which changes nothing but the sign of a zero.
//
// A workgroup stages the whole model in LDS once (the image the host built: per layer W transposed, [unit][k] with a row stride
// of 4 * odd floats so that the 16 units x 4 k of an A read fall in 64 different banks, then the biases; offset and scale) and
// walks tiles of pixels.  A wave owns 16 T pixels (8 waves of T = 2 where that fits LDS beside the model, fewer pixels where it does
// not: rsseg_mlp_plan) and two activation areas of its own, [row = unit][pixel], which the layers write and read in turn: layer l
// reads h_(l-1) from one and writes h_l into the other, so the accumulator tile (units in registers, pixels on lanes) becomes the
// next layer's B operand (k on the lane group) through LDS with k still ascending.  The 16-pixel groups of an area are
// XOR-swizzled (mlp_at) so that the B read (rows g + 4 s over the lane groups g) and the D write (rows 4 g + r) are both free of
// bank conflicts.  Nothing crosses waves after the staging, so the only barrier is the one behind it; inside a wave the LDS
// executes in order and a wavefront fence keeps the compiler from moving a layer's reads above the writes before it.
// The input layer and the epilogue run one pixel per lane (lanes below 16 T).
#include <algorithm>
#include <cmath>

#include "common.h"

#define MLP_MAX_WEIGHT_LAYERS (RSSEG_MLP_MAX_HIDDEN_LAYERS + 1)   // the hidden layers and the output layer
#define MLP_MAX_WIDTH RSSEG_MLP_MAX_WIDTH
#define MLP_MAX_CLASSES RSSEG_MLP_MAX_CLASSES
#define MLP_LDS_BYTES 163840         // one workgroup may take the CU's whole LDS
#define MLP_WAVES 8                  // at most, in a workgroup

typedef float mlp_f4 __attribute__((ext_vector_type(4)));

struct mlp_planes_t {
    const float *p[RSSEG_MAX_FEATURES];
};
struct mlp_desc {
    int L;                                   // layers with weights
    int in[MLP_MAX_WEIGHT_LAYERS];           // inputs of layer l (l = 0 is the first hidden layer)
    int out[MLP_MAX_WEIGHT_LAYERS];          // units
    int ksteps[MLP_MAX_WEIGHT_LAYERS];       // ceil(in / 4)
    int stride[MLP_MAX_WEIGHT_LAYERS];       // floats per row of W transposed: 4 * odd, >= 4 ksteps
    int w_off[MLP_MAX_WEIGHT_LAYERS];        // float offsets into the image
    int b_off[MLP_MAX_WEIGHT_LAYERS];
    int os_off;                              // offset[64] then scale[64], then the k class values as ints
    int image;                               // floats in the image, a multiple of 4
    int rows[2];                             // rows of the two activation areas (area l & 1 holds h_l)
    int F, k, act;
};

// K28's svm_exp, operation for operation (include/rsseg.h)
__device__ __forceinline__ double mlp_exp(double t)
{
    const double LOG2E = __longlong_as_double(0x3FF71547652B82FEll), LN2_HI = __longlong_as_double(0x3FE62E42FEE00000ll),
                 LN2_LO = __longlong_as_double(0x3DEA39EF35793C76ll);
    const bool under = t < -708.0;
    const double tc = under ? -708.0 : t;
    const double n = rint(tc * LOG2E);
    double r = fma(-n, LN2_HI, tc);
    r = fma(-n, LN2_LO, r);
    constexpr double c[14] = {1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0, 1.0 / 362880.0,
                              1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0};
    double p = c[13];
#pragma unroll
    for (int j = 12; j >= 0; j--) p = fma(p, r, c[j]);
    const double two_n = __longlong_as_double((long long)((int)n + 1023) << 52);
    return under ? 0.0 : p * two_n;
}

__device__ __forceinline__ float mlp_activation(float a, int act)   // act is uniform
{
    if (act == RSSEG_MLP_RELU) return a > 0.0f ? a : 0.0f;
    if (act == RSSEG_MLP_IDENTITY) return a;
    const double x = (double)a, ax = fabs(x);
    if (act == RSSEG_MLP_LOGISTIC) {
        const double e = mlp_exp(-ax);
        const double d = 1.0 + e;
        return (float)(x >= 0.0 ? 1.0 / d : e / d);
    }
    if (ax < 0x1p-13) return a;
    const double e = mlp_exp(-(2.0 * ax));
    const double t = (1.0 - e) / (1.0 + e);
    return (float)(x < 0.0 ? -t : t);
}

// the float of [row][px] in an activation area of 16 T pixels per row.  Whatever T, 64 consecutive floats hold four 16-pixel
// groups, and the group is XOR-swizzled so that the four lane groups of a B read (rows g + 4 s) and of a D write (rows 4 g + r)
// fall in four different groups, which makes both free of bank conflicts:
//   T = 4  one row per 64 floats, group t ^ (row & 3) ^ ((row >> 2) & 3)
//   T = 2  two rows per 64 floats, group (2 (row & 1) + t) ^ ((row >> 2) & 3) ^ ((row >> 1) & 1)
//   T = 1  four rows per 64 floats, group (row & 3) ^ ((row >> 2) & 3)
template <int T> __device__ __forceinline__ int mlp_at(int row, int px)
{
    if constexpr (T == 4) return row * 64 + (px ^ ((((row & 3) ^ (row >> 2)) & 3) << 4));
    else if constexpr (T == 2) return (row >> 1) * 64 + ((((((row & 1) << 1) | (px >> 4)) ^ ((row >> 2) & 3) ^ ((row >> 1) & 1)) & 3) << 4) + (px & 15);
    else return (row >> 2) * 64 + ((((row & 3) ^ (row >> 2)) & 3) << 4) + px;
}

// the wave's LDS writes before, its reads after: the hardware keeps a wave's LDS operations in order, the compiler must too
__device__ __forceinline__ void mlp_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one layer of the wave's 16 T pixels: src = h_(l-1), dst = h_l (the activation applied unless it is the output layer)
template <int T>
__device__ __forceinline__ void mlp_layer(const float *__restrict__ wt, const float *__restrict__ bias, int ksteps, int stride, int out, bool hidden,
                                          int act, const float *src, float *dst)
{
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int rows = (out + 3) & ~3;   // the next layer reads rows up to its padded k
    for (int u0 = 0; u0 < out; u0 += 16) {
        const mlp_f4 b4 = *reinterpret_cast<const mlp_f4 *>(bias + u0 + 4 * g);
        mlp_f4 acc[T];
#pragma unroll
        for (int t = 0; t < T; t++) acc[t] = b4;
        const float *wrow = wt + (u0 + c) * stride + g;
        for (int s = 0; s < ksteps; s++) {
            const float a = wrow[4 * s];
#pragma unroll
            for (int t = 0; t < T; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, src[mlp_at<T>(4 * s + g, 16 * t + c)], acc[t], 0, 0, 0);
        }
        const int r0 = u0 + 4 * g;
        if (r0 < rows) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
#pragma unroll
                for (int t = 0; t < T; t++) {
                    float v = acc[t][r];
                    if (hidden) v = mlp_activation(v, act);
                    dst[mlp_at<T>(r0 + r, 16 * t + c)] = r0 + r < out ? v : 0.0f;   // the padding rows are +0, whatever the inputs
                }
            }
        }
    }
}

template <int T>
__global__ __launch_bounds__(64 * MLP_WAVES) void mlp_classify(mlp_planes_t pl, int64_t n, int64_t n_tiles, mlp_desc md, const float *__restrict__ image,
                                                                int waves, uint8_t *__restrict__ labels, float *__restrict__ margin,
                                                                float *__restrict__ conf, float *__restrict__ proba)
{
    constexpr int PX = 16 * T;
    extern __shared__ __attribute__((aligned(16))) float mlp_lds[];
    for (int i = threadIdx.x; i < md.image / 4; i += blockDim.x)
        reinterpret_cast<mlp_f4 *>(mlp_lds)[i] = reinterpret_cast<const mlp_f4 *>(image)[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *area[2];
    area[0] = mlp_lds + md.image + wave * (md.rows[0] + md.rows[1]) * PX;
    area[1] = area[0] + md.rows[0] * PX;
    const float *offs = mlp_lds + md.os_off, *scl = offs + RSSEG_MAX_FEATURES;
    const int *value = reinterpret_cast<const int *>(scl + RSSEG_MAX_FEATURES);
    const int F = md.F, k = md.k, L = md.L;
    const int F4 = (F + 3) & ~3;
    const int tile_px = waves * PX;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t pix = tile * tile_px + (int64_t)wave * PX + lane;
        const bool mine = lane < PX && pix < n;
        bool bad = false;
        if (lane < PX) {   // the input layer: one pixel per lane, 16 planes' loads in flight at a time
            for (int f0 = 0; f0 < F4; f0 += 16) {
                float x[16];
#pragma unroll
                for (int u = 0; u < 16; u++) x[u] = (mine && f0 + u < F) ? __builtin_nontemporal_load(pl.p[f0 + u] + pix) : 0.0f;
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const int f = f0 + u;
                    if (f < F4) {
                        float z = 0.0f;
                        if (f < F) {
                            float v = x[u];
                            if (v != v) v = 0.0f;
                            if (fabsf(v) == INFINITY) {
                                bad = true;
                                v = 0.0f;
                            }
                            z = (v - offs[f]) * scl[f];
                        }
                        area[0][mlp_at<T>(f, lane)] = z;
                    }
                }
            }
        }
        mlp_wave_sync();
        for (int l = 0; l < L; l++) {
            mlp_layer<T>(mlp_lds + md.w_off[l], mlp_lds + md.b_off[l], md.ksteps[l], md.stride[l], md.out[l], l + 1 < L, md.act, area[l & 1],
                         area[(l + 1) & 1]);
            mlp_wave_sync();
        }
        if (mine) {   // the epilogue: one pixel per lane, its logits down a column of the last area
            const float *o = area[L & 1];
            const bool two = k == 2;   // scikit-learn's binary model has one output unit: the logits are (+0, o_0)
            auto logit = [&](int j) -> float { return two ? (j == 0 ? 0.0f : o[mlp_at<T>(0, lane)]) : o[mlp_at<T>(j, lane)]; };
            float best = logit(0);
            int win = 0;
            for (int j = 1; j < k; j++) {
                const float v = logit(j);
                if (v > best || (best != best && v == v)) {
                    best = v;
                    win = j;
                }
            }
            const float qnan = __uint_as_float(0x7fc00000u);
            labels[pix] = (uint8_t)(bad ? 0 : value[win]);
            if (margin) {
                float second = 0.0f;
                bool have = false;
                for (int j = 0; j < k; j++) {
                    if (j == win) continue;
                    const float v = logit(j);
                    if (!have || v > second || (second != second && v == v)) second = v;
                    have = true;
                }
                margin[pix] = bad ? qnan : best - second;
            }
            if (conf || proba) {
                double s = 0.0;
                for (int j = 0; j < k; j++) s = s + mlp_exp((double)logit(j) - (double)best);
                if (conf) conf[pix] = bad ? qnan : (float)(1.0 / s);
                if (proba)
                    for (int j = 0; j < k; j++) proba[(int64_t)j * n + pix] = bad ? qnan : (float)(mlp_exp((double)logit(j) - (double)best) / s);
            }
        }
        mlp_wave_sync();   // the next tile's input layer overwrites what the epilogue read
    }
}

namespace {

struct mlp_plan_t {
    mlp_desc md;
    int T, waves;
    size_t lds_bytes;
};

// the image's layout and the tile that fits beside it; false when the model's limits are exceeded or nothing fits
bool mlp_make_plan(int F, int n_layers, const int *widths, int k, mlp_plan_t &p)
{
    memset(&p, 0, sizeof(p));
    if (F < 1 || F > RSSEG_MAX_FEATURES || n_layers < 2 || n_layers > MLP_MAX_WEIGHT_LAYERS || !widths || k < 2 || k > MLP_MAX_CLASSES) return false;
    if (widths[0] != F || widths[n_layers] != (k == 2 ? 1 : k)) return false;
    for (int l = 1; l < n_layers; l++)
        if (widths[l] < 1 || widths[l] > MLP_MAX_WIDTH) return false;
    mlp_desc &md = p.md;
    md.L = n_layers;
    md.F = F;
    md.k = k;
    int at = 0;
    md.rows[0] = (F + 3) & ~3;
    md.rows[1] = 0;
    for (int l = 0; l < n_layers; l++) {
        md.in[l] = widths[l];
        md.out[l] = widths[l + 1];
        md.ksteps[l] = (widths[l] + 3) / 4;
        md.stride[l] = 4 * (md.ksteps[l] | 1);   // 4 * odd
        const int up = (md.out[l] + 15) & ~15;
        md.w_off[l] = at;
        at += up * md.stride[l];
        md.b_off[l] = at;
        at += up;
        const int rows = (md.out[l] + 3) & ~3;
        if (rows > md.rows[(l + 1) & 1]) md.rows[(l + 1) & 1] = rows;
    }
    md.os_off = at;
    at += 2 * RSSEG_MAX_FEATURES + MLP_MAX_CLASSES;
    md.image = at;
    // (waves, T) in the order of preference: the most pixels in flight, and for as many the most waves (they hide each other's waits)
    const int shapes[][2] = {{8, 2}, {4, 4}, {8, 1}, {4, 2}, {4, 1}, {2, 2}, {2, 1}, {1, 2}, {1, 1}};
    for (const auto &s : shapes) {
        const size_t bytes = sizeof(float) * ((size_t)at + (size_t)s[0] * (md.rows[0] + md.rows[1]) * 16 * s[1]);
        if (bytes <= MLP_LDS_BYTES) {
            p.waves = s[0];
            p.T = s[1];
            p.lds_bytes = bytes;
            return true;
        }
    }
    return false;
}

}  // namespace

extern "C" void rsseg_mlp_plan(int F, int n_layers, const int *widths, int k, int *fits, int *tile_pixels)
{
    mlp_plan_t p;
    const bool ok = mlp_make_plan(F, n_layers, widths, k, p);
    if (fits) *fits = ok ? 1 : 0;
    if (tile_pixels) *tile_pixels = ok ? p.waves * 16 * p.T : 0;
}

extern "C" int rsseg_mlp_classify(rsseg_ctx *ctx, const void *const *d_planes, int F, int64_t n, int n_layers, const int *widths, const float *weights,
                                  const float *biases, const float *offset, const float *scale, int activation, int k, const uint8_t *class_values,
                                  uint8_t *d_labels, float *d_margin, float *d_conf, float *d_proba)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || F < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: d_planes is empty (F=%d)", F);
    if (F > RSSEG_MAX_FEATURES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "mlp_classify: F=%d feature planes, the kernel takes at most %d", F, RSSEG_MAX_FEATURES);
    if (n_layers < 2 || n_layers > MLP_MAX_WEIGHT_LAYERS)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "mlp_classify: n_layers=%d, the kernel takes 1 to %d hidden layers (n_layers 2 to %d)", n_layers,
                       MLP_MAX_WEIGHT_LAYERS - 1, MLP_MAX_WEIGHT_LAYERS);
    if (k < 2) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: k=%d classes, must be >= 2", k);
    if (k > MLP_MAX_CLASSES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "mlp_classify: k=%d classes, the kernel takes at most %d", k, MLP_MAX_CLASSES);
    if (activation != RSSEG_MLP_RELU && activation != RSSEG_MLP_IDENTITY && activation != RSSEG_MLP_LOGISTIC && activation != RSSEG_MLP_TANH)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "mlp_classify: activation=%d, must be RSSEG_MLP_RELU, _IDENTITY, _LOGISTIC or _TANH", activation);
    if (n < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: n=%lld is negative", (long long)n);
    if (!widths || !weights || !biases || !offset || !scale || !class_values)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: the model (widths, weights, biases, offset, scale, class_values) is missing");
    for (int l = 0; l <= n_layers; l++)
        if (widths[l] < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: widths[%d]=%d, must be >= 1", l, widths[l]);
    if (widths[0] != F) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: widths[0]=%d, the call has F=%d planes", widths[0], F);
    for (int l = 1; l < n_layers; l++)
        if (widths[l] > MLP_MAX_WIDTH)
            return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "mlp_classify: widths[%d]=%d, a hidden layer has at most %d units", l, widths[l], MLP_MAX_WIDTH);
    if (widths[n_layers] != (k == 2 ? 1 : k))
        return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: widths[%d]=%d output units, k=%d classes have %d", n_layers, widths[n_layers], k, k == 2 ? 1 : k);
    size_t n_w = 0, n_b = 0;
    for (int l = 0; l < n_layers; l++) {
        n_w += (size_t)widths[l] * widths[l + 1];
        n_b += widths[l + 1];
    }
    auto finite = [&](const char *what, const float *v, size_t count) -> int {
        for (size_t i = 0; i < count; i++)
            if (!std::isfinite(v[i])) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: %s[%lld] is not finite", what, (long long)i);
        return RSSEG_OK;
    };
    RSCHK(finite("offset", offset, F));
    RSCHK(finite("scale", scale, F));
    for (int f = 0; f < F; f++)
        if (scale[f] == 0.0f) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: scale[%d] is 0", f);
    RSCHK(finite("weights", weights, n_w));
    RSCHK(finite("biases", biases, n_b));
    bool seen[256] = {false};
    for (int j = 0; j < k; j++) {
        if (class_values[j] == 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: class_values[%d] is 0, the value of an unclassified pixel", j);
        if (seen[class_values[j]]) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: class_values[%d]=%d occurs twice", j, (int)class_values[j]);
        seen[class_values[j]] = true;
    }
    mlp_plan_t plan;
    if (!mlp_make_plan(F, n_layers, widths, k, plan))
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "mlp_classify: the model's layers do not fit the %d bytes of LDS beside one tile of pixels", MLP_LDS_BYTES);
    if (n == 0) return RSSEG_OK;
    mlp_planes_t pl;
    memset(&pl, 0, sizeof(pl));
    for (int f = 0; f < F; f++) {
        if (!d_planes[f]) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: d_planes[%d] is null", f);
        if ((uintptr_t)d_planes[f] & 3) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: d_planes[%d] is not aligned to its element", f);
        pl.p[f] = reinterpret_cast<const float *>(d_planes[f]);
    }
    if (!d_labels) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: d_labels is null");
    if ((uintptr_t)d_margin & 3) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: d_margin is not aligned to its element");
    if ((uintptr_t)d_conf & 3) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: d_conf is not aligned to its element");
    if ((uintptr_t)d_proba & 3) return rs_fail(ctx, RSSEG_ERR_INVALID, "mlp_classify: d_proba is not aligned to its element");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the image, as the kernel's LDS holds it
    mlp_desc &md = plan.md;
    md.act = activation;
    const size_t bytes = sizeof(float) * (size_t)md.image;
    RSCHK(ws_reserve(ctx, bytes));
    RSCHK(pin_reserve(ctx, bytes));
    float *h = reinterpret_cast<float *>(ctx->h_pin);
    memset(h, 0, bytes);
    const float *w = weights, *b = biases;
    for (int l = 0; l < n_layers; l++) {
        const int in = widths[l], out = widths[l + 1];
        for (int i = 0; i < in; i++)
            for (int u = 0; u < out; u++) h[md.w_off[l] + u * md.stride[l] + i] = w[(size_t)i * out + u];
        memcpy(h + md.b_off[l], b, sizeof(float) * out);
        w += (size_t)in * out;
        b += out;
    }
    memcpy(h + md.os_off, offset, sizeof(float) * F);
    for (int f = 0; f < RSSEG_MAX_FEATURES; f++) h[md.os_off + RSSEG_MAX_FEATURES + f] = f < F ? scale[f] : 1.0f;
    for (int j = 0; j < k; j++) reinterpret_cast<int *>(h + md.os_off + 2 * RSSEG_MAX_FEATURES)[j] = class_values[j];
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_ws, ctx->h_pin, bytes, hipMemcpyHostToDevice, ctx->stream));
    const int tile_px = plan.waves * 16 * plan.T;
    const int64_t n_tiles = ceil_div64(n, tile_px);
    int cus = 0;
    HIPCHK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    const int64_t resident = (int64_t)(cus > 0 ? cus : 1) * (int64_t)std::max<size_t>(1, std::min<size_t>(8, MLP_LDS_BYTES / plan.lds_bytes));
    const dim3 grid((unsigned)std::min<int64_t>(n_tiles, resident)), block(64 * plan.waves);
    const float *image = reinterpret_cast<const float *>(ctx->d_ws);
    {
        prof_scope ps(ctx, "mlp_classify");
        if (plan.T == 4) {
            RSCHK(set_max_dyn_lds(ctx, reinterpret_cast<const void *>(&mlp_classify<4>), plan.lds_bytes));
            hipLaunchKernelGGL((mlp_classify<4>), grid, block, plan.lds_bytes, ctx->stream, pl, n, n_tiles, md, image, plan.waves, d_labels, d_margin, d_conf, d_proba);
        } else if (plan.T == 2) {
            RSCHK(set_max_dyn_lds(ctx, reinterpret_cast<const void *>(&mlp_classify<2>), plan.lds_bytes));
            hipLaunchKernelGGL((mlp_classify<2>), grid, block, plan.lds_bytes, ctx->stream, pl, n, n_tiles, md, image, plan.waves, d_labels, d_margin, d_conf, d_proba);
        } else {
            RSCHK(set_max_dyn_lds(ctx, reinterpret_cast<const void *>(&mlp_classify<1>), plan.lds_bytes));
            hipLaunchKernelGGL((mlp_classify<1>), grid, block, plan.lds_bytes, ctx->stream, pl, n, n_tiles, md, image, plan.waves, d_labels, d_margin, d_conf, d_proba);
        }
        HIPCHK(ctx, hipGetLastError());
    }
    // the upload has to have left the pinned area before the next call writes into it
    HIPCHK(ctx, rs_sync(ctx));
    return RSSEG_OK;
}
