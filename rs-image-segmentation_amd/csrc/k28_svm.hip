// K28 — rsseg_svm_classify: support vector machine classification (one-vs-one, libsvm's decision rule) of feature-planar
// rasters.  One per-pixel sweep: a kernel value per support vector, the P = k (k - 1) / 2 pair sums open across that loop, then
// the vote.  The arithmetic is the restatement's (tests/svm_ref.py), operation for operation, in float64:
//   x_f  = the plane value widened (exact), a NaN read as 0; a pixel with any +-inf x_f gets label 0 and margin NaN
//   z_f  = (x_f - offset_f) * scale_f
//   RBF     q = fma chain over f of d * d, d = z_f - sv_if, from +0;  K_i = svm_exp(-(gamma * q))
//   POLY    t = fma chain over f of sv_if * z_f from +0;  u = fma(gamma, t, coef0);  K_i = u * u * ... (degree factors)
//   LINEAR  d_p = (fma chain over f of w_pf * z_f from +0) + bias_p: no loop over support vectors
//   pairs p = (a, b), a < b, in the order (0,1), (0,2), ..., (k-2,k-1):  s = fma chain of coef[b-1][i] * K_i over class a's
//   support vectors, then of coef[a][i] * K_i over class b's, from +0;  d_p = s + bias_p;  d_p > 0 votes a, else b
//   label = the lowest class with the most votes;  margin = float32(min |d_p| over the winner's pairs), a NaN never the min
// fma() stands where the restatement has one and nowhere else (the file is built with -ffp-contract=off like the rest).
//
// The support vectors are grouped by class, classes ascending, so ONE ascending sweep over them feeds every pair in its own
// order: a vector of class c adds coef[r][i] * K_i to the pair of c and o = r + (r >= c), for r = 0 .. k-2.
// Registers.  A lane keeps z of its G pixels (two; one at FR = 64 and in the LDS form) in float64 for the whole loop.  FR
// (compile time: 4, 8, 16, 24, 32, 64) is the smallest width that holds F; columns at or beyond F are skipped by uniform
// branches where a plane is read.  The loop over support vectors, the class of a vector, its row and its k - 1 coefficients
// are wave-uniform: scalar loads from the model's copy in the workspace, no per-lane gather.  A vector's row there is its F
// features, zeros up to FR, then its k - 1 coefficients and zeros up to 8 (16 in the LDS form): one contiguous run, read by
// straight-line code.  The padding is bit-neutral: z is +0 from F on, so the RBF's fma(0, 0, q) and the polynomial's
// fma(0, 0, t) return q and t themselves (neither is ever -0), and a zero coefficient only feeds the sum of a pair whose class
// the call does not have, which nothing reads.  SV_UNROLL vectors of one class are evaluated together (independent fma
// chains), then added in ascending order.
// Pair sums.  k <= 8: acc[28][G] in registers, indexed by the pair's slot in the 8-class triangle; the class of the vector
// selects (a uniform switch) the statically indexed update.  k = 9 .. 16: one pixel per lane and the P sums of a lane in its
// own LDS column (P x 64 doubles per one-wave workgroup, sized by the call's k), the same updates with uniform indices.
// MFMA is not used: the order in which v_mfma_f64_16x16x4_f64 adds its four products is not documented as this fma chain.
#include <cmath>
#include <type_traits>

#include "common.h"

#define SV_THREADS 256       // register form and LINEAR
#define SV_LDS_THREADS 64    // LDS form: one wave, one pixel per lane
#define SV_UNROLL 2          // support vectors of one class evaluated together
#define SV_KREG 8            // classes whose pair sums live in registers
#define SV_PREG (SV_KREG * (SV_KREG - 1) / 2)

struct sv_planes_t {
    const void *p[RSSEG_MAX_FEATURES];
};
struct sv_model_t {
    const double *offset;   // [F]
    const double *scale;    // [F]
    const double *rows;     // [S][FR + CP]: a support vector's F features, zeros up to FR, then its k - 1 coefficients, zeros up to CP
    const double *bias;     // [P]
    const double *w;        // [P][FR], LINEAR: zeros from F on
    const int *start;       // [k + 1] first support vector of every class
    const int *value;       // [k] class values, 1..255
    int degree;
    double gamma, coef0;
};

// exp(t) for t <= 0 as a fixed sequence of float64 operations (include/rsseg.h has the contract)
__device__ __forceinline__ double svm_exp(double t)
{
    const double LOG2E = __longlong_as_double(0x3FF71547652B82FEll), LN2_HI = __longlong_as_double(0x3FE62E42FEE00000ll),
                 LN2_LO = __longlong_as_double(0x3DEA39EF35793C76ll);
    const bool under = t < -708.0;
    const double tc = under ? -708.0 : t;   // keeps n in range on the lanes whose result is +0 anyway
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

constexpr int sv_slot(int a, int b) { return a * SV_KREG - a * (a + 1) / 2 + (b - a - 1); }   // a < b < SV_KREG

// K of one support vector (its row of F scaled features) at the lane's G pixels
template <int KERNEL, int FR, int G>
__device__ __forceinline__ void sv_value(const double (&z)[FR][G], const double *__restrict__ row, const sv_model_t &md, double (&K)[G])
{
    double s[G];
#pragma unroll
    for (int g = 0; g < G; g++) s[g] = 0.0;
#pragma unroll
    for (int f = 0; f < FR; f++) {   // columns from F on hold zeros in the row and in z: fma(0, 0, s) is s, bit for bit
        const double v = row[f];
#pragma unroll
        for (int g = 0; g < G; g++) {
            if constexpr (KERNEL == RSSEG_SVM_RBF) {
                const double d = z[f][g] - v;
                s[g] = fma(d, d, s[g]);
            } else {
                s[g] = fma(v, z[f][g], s[g]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
        if constexpr (KERNEL == RSSEG_SVM_RBF) {
            K[g] = svm_exp(-(md.gamma * s[g]));
        } else {
            const double u = fma(md.gamma, s[g], md.coef0);
            double v = u;
            for (int j = 1; j < md.degree; j++) v = v * u;
            K[g] = v;
        }
    }
}

// a support vector of class C adds coef[r][i] * K to the pair of C and o = r + (r >= C): registers, static slots
template <int C, int G>
__device__ __forceinline__ void sv_add_class(double (&acc)[SV_PREG][G], const double *__restrict__ coef_i, const double (&K)[G])
{
#pragma unroll
    for (int r = 0; r < SV_KREG - 1; r++) {   // rows from k - 1 on hold zeros and feed slots of classes the call does not have: never read
        const int o = r + (r >= C ? 1 : 0);
        const int slot = C < o ? sv_slot(C, o) : sv_slot(o, C);
        const double cf = coef_i[r];
#pragma unroll
        for (int g = 0; g < G; g++) acc[slot][g] = fma(cf, K[g], acc[slot][g]);
    }
    // ends the case of sv_add_regs' switch with something the optimiser will not merge across cases: merged, the cases' stores
    // would share one address chosen by the class, and the sums it covers would leave the registers for scratch memory
    asm volatile("");
}

template <int G>
__device__ __forceinline__ void sv_add_regs(double (&acc)[SV_PREG][G], int c, const double *__restrict__ coef_i, const double (&K)[G])
{
    switch (c) {   // uniform
    case 0: sv_add_class<0, G>(acc, coef_i, K); break;
    case 1: sv_add_class<1, G>(acc, coef_i, K); break;
    case 2: sv_add_class<2, G>(acc, coef_i, K); break;
    case 3: sv_add_class<3, G>(acc, coef_i, K); break;
    case 4: sv_add_class<4, G>(acc, coef_i, K); break;
    case 5: sv_add_class<5, G>(acc, coef_i, K); break;
    case 6: sv_add_class<6, G>(acc, coef_i, K); break;
    default: sv_add_class<7, G>(acc, coef_i, K); break;
    }
}

// the same update on the lane's LDS column: col[p * SV_LDS_THREADS], p the pair's index among the call's k classes
__device__ __forceinline__ void sv_add_lds(double *col, int c, int k, const double *__restrict__ coef_i, double K)
{
    for (int r = 0; r < k - 1; r++) {
        const int o = r + (r >= c ? 1 : 0);
        const int a = c < o ? c : o, b = c < o ? o : c;
        const int p = a * k - a * (a + 1) / 2 + (b - a - 1);
        col[p * SV_LDS_THREADS] = fma(coef_i[r], K, col[p * SV_LDS_THREADS]);
    }
}

// one support vector's kernel value into the pair sums of its class: the registers, or the lane's LDS column
template <bool LDS, int G, int PR>
__device__ __forceinline__ void sv_add(double (&acc)[PR][G], double *col, int c, int k, const double *__restrict__ coef_i, const double (&K)[G])
{
    if constexpr (LDS) sv_add_lds(col, c, k, coef_i, K[0]);
    else sv_add_regs<G>(acc, c, coef_i, K);
}

// votes: 4 bits per class (a class takes at most k - 1 <= 15)
__device__ __forceinline__ void sv_vote(unsigned long long &votes, double d, int a, int b) { votes += 1ull << (4 * (d > 0.0 ? a : b)); }

__device__ __forceinline__ void sv_winner(unsigned long long votes, int k, const int *__restrict__ value, int &win, int &winv)
{
    int best = -1;
    win = winv = 0;
    for (int c = 0; c < k; c++) {
        const int cnt = (int)((votes >> (4 * c)) & 15ull);
        const int cv = value[c];
        if (cnt > best) {
            best = cnt;
            win = c;
            winv = cv;
        }
    }
}

// the lane's G pixels: z, and whether any plane holds +-inf there
template <typename T, int FR, int G>
__device__ __forceinline__ void sv_load(const sv_planes_t &pl, int F, int64_t base, int64_t n, int vec, const sv_model_t &md, double (&z)[FR][G], bool (&bad)[G])
{
    const bool whole = base + G <= n;
#pragma unroll
    for (int g = 0; g < G; g++) bad[g] = false;
#pragma unroll
    for (int f = 0; f < FR; f++) {
        if (f < F) {
            const T *__restrict__ src = reinterpret_cast<const T *>(pl.p[f]);
            T x[G];
            bool wide = false;
            if constexpr (G == 2) {   // both pixels in one load where every plane is aligned to it
                wide = whole && (vec & 1);
                if (wide) {
                    using V = std::conditional_t<sizeof(T) == 4, uint2, uint4>;
                    const V raw = *reinterpret_cast<const V *>(src + base);
                    memcpy(x, &raw, sizeof(V));
                }
            }
            if (!wide) {
#pragma unroll
                for (int g = 0; g < G; g++) x[g] = base + g < n ? src[base + g] : (T)0;
            }
            const double off = md.offset[f], sc = md.scale[f];
#pragma unroll
            for (int g = 0; g < G; g++) {
                double xv = (double)x[g];
                if (xv != xv) xv = 0.0;
                if (fabs(xv) == (double)INFINITY) {
                    bad[g] = true;
                    xv = 0.0;
                }
                z[f][g] = (xv - off) * sc;
            }
        } else {
#pragma unroll
            for (int g = 0; g < G; g++) z[f][g] = 0.0;
        }
    }
}

template <int G>
__device__ __forceinline__ void sv_store(int64_t base, int64_t n, int vec, const uint8_t (&lab)[G], const float (&mv)[G], uint8_t *__restrict__ labels,
                                         float *__restrict__ margin)
{
    const bool whole = base + G <= n;
    if (G == 2 && whole && (vec & 2)) {
        uint16_t v;
        memcpy(&v, lab, 2);
        *reinterpret_cast<uint16_t *>(labels + base) = v;
    } else {
#pragma unroll
        for (int g = 0; g < G; g++)
            if (base + g < n) labels[base + g] = lab[g];
    }
    if (margin) {
        if (G == 2 && whole && (vec & 4)) {
            *reinterpret_cast<float2 *>(margin + base) = make_float2(mv[0], mv[G - 1]);
        } else {
#pragma unroll
            for (int g = 0; g < G; g++)
                if (base + g < n) margin[base + g] = mv[g];
        }
    }
}

template <int FR, bool LDS> struct sv_shape {
    static constexpr int G = (LDS || FR > 32) ? 1 : 2;   // pixels per lane
    static constexpr int THREADS = LDS ? SV_LDS_THREADS : SV_THREADS;
    static constexpr int CP = LDS ? RSSEG_SVM_MAX_CLASSES : SV_KREG;   // coefficient slots of a row (k - 1 used)
    static constexpr int ROW = FR + CP;                                // doubles per support vector
};

template <typename T, int FR, int KERNEL, bool LDS>
__global__ __launch_bounds__(LDS ? SV_LDS_THREADS : SV_THREADS) void svm_classify(sv_planes_t pl, int F, int k, int64_t n, sv_model_t md, int vec,
                                                                                    uint8_t *__restrict__ labels, float *__restrict__ margin)
{
    constexpr int G = sv_shape<FR, LDS>::G, THREADS = sv_shape<FR, LDS>::THREADS, ROW = sv_shape<FR, LDS>::ROW;
    extern __shared__ double sv_lds[];   // LDS form: [P][SV_LDS_THREADS]
    const int64_t base = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * G;
    if (base >= n) return;   // no barrier below: a lane's LDS column is its own
    double z[FR][G];
    bool bad[G];
    sv_load<T, FR, G>(pl, F, base, n, vec, md, z, bad);
    const int P = k * (k - 1) / 2;
    double acc[LDS ? 1 : SV_PREG][G];
    double *col = sv_lds + threadIdx.x;
    if constexpr (LDS) {
        for (int p = 0; p < P; p++) col[p * SV_LDS_THREADS] = 0.0;
    } else {
#pragma unroll
        for (int s = 0; s < SV_PREG; s++)
#pragma unroll
            for (int g = 0; g < G; g++) acc[s][g] = 0.0;
    }
    for (int c = 0; c < k; c++) {
        const int lo = md.start[c], hi = md.start[c + 1];
        int i = lo;
        for (; i + SV_UNROLL <= hi; i += SV_UNROLL) {
            double K[SV_UNROLL][G];
#pragma unroll
            for (int u = 0; u < SV_UNROLL; u++) sv_value<KERNEL, FR, G>(z, md.rows + (size_t)(i + u) * ROW, md, K[u]);
#pragma unroll
            for (int u = 0; u < SV_UNROLL; u++) sv_add<LDS, G>(acc, col, c, k, md.rows + (size_t)(i + u) * ROW + FR, K[u]);
        }
        for (; i < hi; i++) {
            double K[G];
            sv_value<KERNEL, FR, G>(z, md.rows + (size_t)i * ROW, md, K);
            sv_add<LDS, G>(acc, col, c, k, md.rows + (size_t)i * ROW + FR, K);
        }
    }
    // decisions (kept where the sums were), votes, winner, margin
    unsigned long long votes[G];
#pragma unroll
    for (int g = 0; g < G; g++) votes[g] = 0ull;
    if constexpr (LDS) {
        int p = 0;
        for (int a = 0; a < k - 1; a++)
            for (int b = a + 1; b < k; b++, p++) {
                const double d = col[p * SV_LDS_THREADS] + md.bias[p];
                col[p * SV_LDS_THREADS] = d;
                sv_vote(votes[0], d, a, b);
            }
    } else {
        int p = 0;
#pragma unroll
        for (int a = 0; a < SV_KREG - 1; a++)
#pragma unroll
            for (int b = a + 1; b < SV_KREG; b++) {
                if (b < k) {
                    const double bp = md.bias[p++];
#pragma unroll
                    for (int g = 0; g < G; g++) {
                        const double d = acc[sv_slot(a, b)][g] + bp;
                        acc[sv_slot(a, b)][g] = d;
                        sv_vote(votes[g], d, a, b);
                    }
                }
            }
    }
    uint8_t lab[G];
    float mv[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        int win, winv;
        sv_winner(votes[g], k, md.value, win, winv);
        double m = (double)INFINITY;
        if (margin) {
            if constexpr (LDS) {
                int p = 0;
                for (int a = 0; a < k - 1; a++)
                    for (int b = a + 1; b < k; b++, p++) {
                        const double ad = fabs(col[p * SV_LDS_THREADS]);
                        if ((win == a || win == b) && ad < m) m = ad;
                    }
            } else {
#pragma unroll
                for (int a = 0; a < SV_KREG - 1; a++)
#pragma unroll
                    for (int b = a + 1; b < SV_KREG; b++) {
                        if (b < k) {
                            const double ad = fabs(acc[sv_slot(a, b)][g]);
                            if ((win == a || win == b) && ad < m) m = ad;
                        }
                    }
            }
        }
        lab[g] = (uint8_t)(bad[g] ? 0 : winv);
        mv[g] = bad[g] ? __uint_as_float(0x7fc00000u) : (float)m;
    }
    sv_store<G>(base, n, vec, lab, mv, labels, margin);
}

// LINEAR: the folded weights, one fma chain per pair; the margin pass evaluates the pairs again (the same operations)
template <typename T, int FR>
__global__ __launch_bounds__(SV_THREADS) void svm_classify_linear(sv_planes_t pl, int F, int k, int64_t n, sv_model_t md, int vec,
                                                                  uint8_t *__restrict__ labels, float *__restrict__ margin)
{
    constexpr int G = sv_shape<FR, false>::G;
    const int64_t base = ((int64_t)blockIdx.x * SV_THREADS + threadIdx.x) * G;
    if (base >= n) return;
    double z[FR][G];
    bool bad[G];
    sv_load<T, FR, G>(pl, F, base, n, vec, md, z, bad);
    auto decision = [&](int p, double (&d)[G]) {
        const double *__restrict__ wr = md.w + (size_t)p * FR;
#pragma unroll
        for (int g = 0; g < G; g++) d[g] = 0.0;
#pragma unroll
        for (int f = 0; f < FR; f++) {   // zeros from F on, in w and in z
            const double v = wr[f];
#pragma unroll
            for (int g = 0; g < G; g++) d[g] = fma(v, z[f][g], d[g]);
        }
        const double bp = md.bias[p];
#pragma unroll
        for (int g = 0; g < G; g++) d[g] = d[g] + bp;
    };
    unsigned long long votes[G];
#pragma unroll
    for (int g = 0; g < G; g++) votes[g] = 0ull;
    int p = 0;
    for (int a = 0; a < k - 1; a++)
        for (int b = a + 1; b < k; b++, p++) {
            double d[G];
            decision(p, d);
#pragma unroll
            for (int g = 0; g < G; g++) sv_vote(votes[g], d[g], a, b);
        }
    int win[G], winv[G];
    double m[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        sv_winner(votes[g], k, md.value, win[g], winv[g]);
        m[g] = (double)INFINITY;
    }
    if (margin) {
        p = 0;
        for (int a = 0; a < k - 1; a++)
            for (int b = a + 1; b < k; b++, p++) {
                double d[G];
                decision(p, d);
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const double ad = fabs(d[g]);
                    if ((win[g] == a || win[g] == b) && ad < m[g]) m[g] = ad;
                }
            }
    }
    uint8_t lab[G];
    float mv[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
        lab[g] = (uint8_t)(bad[g] ? 0 : winv[g]);
        mv[g] = bad[g] ? __uint_as_float(0x7fc00000u) : (float)m[g];
    }
    sv_store<G>(base, n, vec, lab, mv, labels, margin);
}

namespace {

constexpr int sv_width(int F) { return F <= 4 ? 4 : F <= 8 ? 8 : F <= 16 ? 16 : F <= 24 ? 24 : F <= 32 ? 32 : 64; }

template <typename T, int FR>
int sv_launch_width(rsseg_ctx *ctx, int kernel, sv_planes_t pl, int F, int k, int64_t n, sv_model_t md, uintptr_t planes_or, uint8_t *labels, float *margin)
{
    const bool lds = kernel != RSSEG_SVM_LINEAR && k > SV_KREG;
    const int G = lds ? 1 : sv_shape<FR, false>::G, threads = lds ? SV_LDS_THREADS : SV_THREADS;
    const int64_t blocks = ceil_div64(n, (int64_t)threads * G);
    if (blocks > 0x7fffffff) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "svm_classify: n=%lld pixels need more than 2^31 - 1 workgroups", (long long)n);
    // which accesses may be G elements wide: planes (G elements), labels (G bytes), margin (4 G bytes)
    const int vec = ((planes_or & (G * sizeof(T) - 1)) == 0 ? 1 : 0) | (((uintptr_t)labels & (G - 1)) == 0 ? 2 : 0) |
                    (((uintptr_t)margin & (4 * G - 1)) == 0 ? 4 : 0);
    const dim3 grid((unsigned)blocks), block(threads);
    const size_t shared = lds ? sizeof(double) * SV_LDS_THREADS * (size_t)(k * (k - 1) / 2) : 0;
    if (kernel == RSSEG_SVM_LINEAR) hipLaunchKernelGGL((svm_classify_linear<T, FR>), grid, block, 0, ctx->stream, pl, F, k, n, md, vec, labels, margin);
    else if (kernel == RSSEG_SVM_RBF && !lds)
        hipLaunchKernelGGL((svm_classify<T, FR, RSSEG_SVM_RBF, false>), grid, block, shared, ctx->stream, pl, F, k, n, md, vec, labels, margin);
    else if (kernel == RSSEG_SVM_RBF)
        hipLaunchKernelGGL((svm_classify<T, FR, RSSEG_SVM_RBF, true>), grid, block, shared, ctx->stream, pl, F, k, n, md, vec, labels, margin);
    else if (!lds)
        hipLaunchKernelGGL((svm_classify<T, FR, RSSEG_SVM_POLY, false>), grid, block, shared, ctx->stream, pl, F, k, n, md, vec, labels, margin);
    else
        hipLaunchKernelGGL((svm_classify<T, FR, RSSEG_SVM_POLY, true>), grid, block, shared, ctx->stream, pl, F, k, n, md, vec, labels, margin);
    return RSSEG_OK;
}

template <typename T, typename... A> int sv_launch(rsseg_ctx *ctx, int F, A... a)
{
    switch (sv_width(F)) {
    case 4: return sv_launch_width<T, 4>(ctx, a...);
    case 8: return sv_launch_width<T, 8>(ctx, a...);
    case 16: return sv_launch_width<T, 16>(ctx, a...);
    case 24: return sv_launch_width<T, 24>(ctx, a...);
    case 32: return sv_launch_width<T, 32>(ctx, a...);
    default: return sv_launch_width<T, 64>(ctx, a...);
    }
}

}  // namespace

// the LINEAR kernel's weights: per pair the fma chain, in the decision's order, of coef * sv_if (host; std::fma is one rounding)
extern "C" int rsseg_host_svm_fold_linear(int F, int k, int S, const double *sv, const int *n_support, const double *coef, double *w)
{
    if (F < 1 || k < 2 || S < 1 || !sv || !n_support || !coef || !w) return RSSEG_ERR_INVALID;
    int start[RSSEG_SVM_MAX_CLASSES + 1];
    if (k > RSSEG_SVM_MAX_CLASSES) return RSSEG_ERR_UNSUPPORTED;
    start[0] = 0;
    for (int j = 0; j < k; j++) {
        if (n_support[j] < 1) return RSSEG_ERR_INVALID;
        start[j + 1] = start[j] + n_support[j];
    }
    if (start[k] != S) return RSSEG_ERR_INVALID;
    int p = 0;
    for (int a = 0; a < k - 1; a++)
        for (int b = a + 1; b < k; b++, p++)
            for (int f = 0; f < F; f++) {
                double t = 0.0;
                for (int i = start[a]; i < start[a + 1]; i++) t = std::fma(coef[(size_t)(b - 1) * S + i], sv[(size_t)i * F + f], t);
                for (int i = start[b]; i < start[b + 1]; i++) t = std::fma(coef[(size_t)a * S + i], sv[(size_t)i * F + f], t);
                w[(size_t)p * F + f] = t;
            }
    return RSSEG_OK;
}

extern "C" int rsseg_svm_classify(rsseg_ctx *ctx, const void *const *d_planes, int F, int dtype, int64_t n, int k, int S, const double *offset,
                                  const double *scale, const double *sv, const int *n_support, const double *coef, const double *bias,
                                  const uint8_t *class_values, int kernel, double gamma, double coef0, int degree, const double *w, uint8_t *d_labels,
                                  float *d_margin)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_planes || F < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: d_planes is empty (F=%d)", F);
    if (F > RSSEG_MAX_FEATURES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "svm_classify: F=%d feature planes, the kernels take at most %d", F, RSSEG_MAX_FEATURES);
    if (k < 2) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: k=%d classes, must be >= 2", k);
    if (k > RSSEG_SVM_MAX_CLASSES) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "svm_classify: k=%d classes, the kernels take at most %d", k, RSSEG_SVM_MAX_CLASSES);
    if (S < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: S=%d support vectors, must be >= 1", S);
    if (S > RSSEG_SVM_MAX_SV) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "svm_classify: S=%d support vectors, the kernels take at most %d", S, RSSEG_SVM_MAX_SV);
    if (dtype != RSSEG_F32 && dtype != RSSEG_F64) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: dtype must be RSSEG_F32 or RSSEG_F64");
    if (n < 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: n=%lld is negative", (long long)n);
    if (kernel != RSSEG_SVM_RBF && kernel != RSSEG_SVM_POLY && kernel != RSSEG_SVM_LINEAR)
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "svm_classify: kernel=%d, must be RSSEG_SVM_RBF, RSSEG_SVM_POLY or RSSEG_SVM_LINEAR", kernel);
    if (!offset || !scale || !sv || !n_support || !coef || !bias || !class_values)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: the model (offset, scale, sv, n_support, coef, bias, class_values) is missing");
    if (kernel == RSSEG_SVM_LINEAR && !w) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: the linear kernel needs the folded weights w");
    const int P = k * (k - 1) / 2;
    auto finite = [&](const char *what, const double *v, size_t count) -> int {
        for (size_t i = 0; i < count; i++)
            if (!std::isfinite(v[i])) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: %s[%lld] is not finite", what, (long long)i);
        return RSSEG_OK;
    };
    RSCHK(finite("offset", offset, F));
    RSCHK(finite("scale", scale, F));
    for (int f = 0; f < F; f++)
        if (scale[f] == 0.0) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: scale[%d] is 0", f);
    RSCHK(finite("sv", sv, (size_t)S * F));
    RSCHK(finite("coef", coef, (size_t)(k - 1) * S));
    RSCHK(finite("bias", bias, P));
    if (kernel == RSSEG_SVM_LINEAR) RSCHK(finite("w", w, (size_t)P * F));
    int64_t total = 0;
    for (int j = 0; j < k; j++) {
        if (n_support[j] < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: n_support[%d]=%d, every class needs a support vector", j, n_support[j]);
        total += n_support[j];
    }
    if (total != S) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: n_support sums to %lld, S=%d", (long long)total, S);
    bool seen[256] = {false};
    for (int j = 0; j < k; j++) {
        if (class_values[j] == 0) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: class_values[%d] is 0, the value of an unclassified pixel", j);
        if (seen[class_values[j]]) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: class_values[%d]=%d occurs twice", j, (int)class_values[j]);
        seen[class_values[j]] = true;
    }
    if (kernel == RSSEG_SVM_RBF && !(std::isfinite(gamma) && gamma > 0.0)) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: gamma=%g, the RBF kernel needs a finite gamma > 0", gamma);
    if (kernel == RSSEG_SVM_POLY) {
        if (!std::isfinite(gamma)) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: gamma is not finite");
        if (!std::isfinite(coef0)) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: coef0 is not finite");
        if (degree < 1) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: degree=%d, must be >= 1", degree);
        if (degree > RSSEG_SVM_MAX_DEGREE) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "svm_classify: degree=%d, the kernels take at most %d", degree, RSSEG_SVM_MAX_DEGREE);
    }
    if (n == 0) return RSSEG_OK;
    const size_t eb = dtype == RSSEG_F32 ? 4 : 8;
    sv_planes_t pl;
    memset(&pl, 0, sizeof(pl));
    uintptr_t planes_or = 0;
    for (int f = 0; f < F; f++) {
        if (!d_planes[f]) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: d_planes[%d] is null", f);
        if ((uintptr_t)d_planes[f] & (eb - 1)) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: d_planes[%d] is not aligned to its element", f);
        pl.p[f] = d_planes[f];
        planes_or |= (uintptr_t)d_planes[f];
    }
    if (!d_labels) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: d_labels is null");
    if ((uintptr_t)d_margin & 3) return rs_fail(ctx, RSSEG_ERR_INVALID, "svm_classify: d_margin is not aligned to its element");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // the model as the kernels read it, uploaded in one copy: offset, scale, bias (float64); per support vector a row of its F
    // features, zeros up to the kernel's width FR, its k - 1 coefficients and zeros up to CP (LINEAR: per pair a row of w, zeros
    // up to FR); then the classes' first vectors and the class values as ints
    const bool linear = kernel == RSSEG_SVM_LINEAR, lds = !linear && k > SV_KREG;
    const int FR = sv_width(F), CP = lds ? RSSEG_SVM_MAX_CLASSES : SV_KREG, ROW = FR + CP;
    const size_t n_rows = linear ? (size_t)P * FR : (size_t)S * ROW;
    const size_t n_dbl = 2 * (size_t)F + (size_t)P + n_rows;
    const size_t bytes = sizeof(double) * n_dbl + sizeof(int) * (size_t)(2 * k + 1);
    RSCHK(ws_reserve(ctx, bytes));
    RSCHK(pin_reserve(ctx, bytes));
    double *h = reinterpret_cast<double *>(ctx->h_pin);
    const double *d = reinterpret_cast<const double *>(ctx->d_ws);
    sv_model_t md;
    memcpy(h, offset, sizeof(double) * F);
    memcpy(h + F, scale, sizeof(double) * F);
    memcpy(h + 2 * F, bias, sizeof(double) * P);
    double *hr = h + 2 * F + P;
    memset(hr, 0, sizeof(double) * n_rows);
    if (linear) {
        for (int p = 0; p < P; p++) memcpy(hr + (size_t)p * FR, w + (size_t)p * F, sizeof(double) * F);
    } else {
        for (int i = 0; i < S; i++) {
            memcpy(hr + (size_t)i * ROW, sv + (size_t)i * F, sizeof(double) * F);
            for (int r = 0; r < k - 1; r++) hr[(size_t)i * ROW + FR + r] = coef[(size_t)r * S + i];
        }
    }
    md.offset = d;
    md.scale = d + F;
    md.bias = d + 2 * F;
    md.rows = md.w = d + 2 * F + P;
    int *hi = reinterpret_cast<int *>(h + n_dbl);
    hi[0] = 0;
    for (int j = 0; j < k; j++) hi[j + 1] = hi[j] + n_support[j];
    for (int j = 0; j < k; j++) hi[k + 1 + j] = class_values[j];
    md.start = reinterpret_cast<const int *>(d + n_dbl);
    md.value = md.start + k + 1;
    md.degree = degree;
    md.gamma = gamma;
    md.coef0 = coef0;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_ws, ctx->h_pin, bytes, hipMemcpyHostToDevice, ctx->stream));
    {
        prof_scope ps(ctx, "svm_classify");
        if (dtype == RSSEG_F32) RSCHK(sv_launch<float>(ctx, F, kernel, pl, F, k, n, md, planes_or, d_labels, d_margin));
        else RSCHK(sv_launch<double>(ctx, F, kernel, pl, F, k, n, md, planes_or, d_labels, d_margin));
        HIPCHK(ctx, hipGetLastError());
    }
    // the upload has to have left the pinned area before the next call writes into it
    HIPCHK(ctx, rs_sync(ctx));
    return RSSEG_OK;
}
