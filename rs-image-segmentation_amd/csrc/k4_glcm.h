// K4 — what the GLCM kernels of k4_glcm.hip (the four default angles) and k4_glcm_offsets.hip (any offsets) share:
// the property maps, the float64 finish over the common denominators of the four default angles, and the exact
// conversion of a fixed-point homogeneity sum to double.
#pragma once
#include "common.h"

struct glcm_out {
    float *p[5];  // contrast, dissimilarity, homogeneity, energy, correlation
};

struct glcm_stats {
    long long np, S1, S2, Hq, M1, M2, Mx, A;
};

// correlation of one angle from exact integers (oracle.c mode 1)
__device__ __forceinline__ double glcm_corr(long long np, long long M1, long long M2, long long Mx)
{
    const long long den = M2 * (2 * np) - M1 * M1, num = Mx * (2 * np) - M1 * M1;
    return den == 0 ? 1.0 : (double)num / (double)den;
}

// The register kernels (one window of WIN <= 7 per finish, grey levels < LV <= 64) take the same integers in 32 bits: with
// np <= WIN (WIN - 1) pairs per angle, M1 <= 2 np (LV - 1), and M2 * 2 np, Mx * 2 np <= 2 np (LV - 1)^2 * 2 np = the bound
// on M1^2; the contrast / dissimilarity numerators S * nb + S' * na <= 4 na nb (LV - 1)^2 are below it too.  WIN = 7,
// LV = 64: 28 005 264 < 2^25, so every product and difference below is exact in int and converts with one v_cvt_f64_i32.
template <int WIN, int LV> constexpr bool glcm_fits_int32()
{
    const long long m1 = 2ll * WIN * (WIN - 1) * (LV - 1);
    return m1 * m1 < (1ll << 31);
}
__device__ __forceinline__ double glcm_corr32(int np, int M1, int M2, int Mx)
{
    const int den = M2 * (2 * np) - M1 * M1, num = Mx * (2 * np) - M1 * M1;
    return den == 0 ? 1.0 : (double)num / (double)den;
}

// group sums: g0 = angles 0 and 90 degrees (na pairs each), g1 = 45 and 135 degrees (nb pairs each)
struct glcm_group {
    long long S1, S2, Hq;
    double sq;  // sqrt(A_a) + sqrt(A_b)
};

// A homogeneity sum of 2^-52 fixed-point terms, split so that no window size overflows it: value = hi * 2^26 + lo.
// A term is at most 2^52 (hq[0]), so hi grows by at most 2^26 and lo by less than 2^26 per pair: exact in int64 for any
// pair count below 2^37.  The int64 sum of the terms themselves overflows once a sum holds more than 2048 pairs of
// equal grey levels (two angles of a smooth window 33 x 33).
#define GLCM_HQ_SPLIT 26
struct glcm_hq_sum {
    long long hi, lo;
};
__device__ __forceinline__ void hq_add(glcm_hq_sum &s, long long term)
{
    s.hi += term >> GLCM_HQ_SPLIT;
    s.lo += term & ((1ll << GLCM_HQ_SPLIT) - 1);
}
// a per-lane int64 partial (exact while the lane holds fewer than 2048 terms) folded into a split sum
__device__ __forceinline__ glcm_hq_sum hq_split(long long partial)
{
    return glcm_hq_sum{partial >> GLCM_HQ_SPLIT, partial & ((1ll << GLCM_HQ_SPLIT) - 1)};
}
// the correctly rounded double of hi * 2^26 + lo (hi, lo >= 0): with value = hh * 2^52 + m, m < 2^52, both hh * 2^52
// and m are exact doubles, so their one addition rounds the exact value once.  Wherever the value fits int64 this is
// the double (double)(int64)value gives: the unsplit sums of the earlier kernels are reproduced bit for bit.
__device__ __forceinline__ double hq_to_double(glcm_hq_sum s)
{
    const long long mask = (1ll << GLCM_HQ_SPLIT) - 1;
    const long long hi = s.hi + (s.lo >> GLCM_HQ_SPLIT), lo = s.lo & mask;
    const long long hh = hi >> GLCM_HQ_SPLIT, m = ((hi & mask) << GLCM_HQ_SPLIT) | lo;
    return (double)hh * 4503599627370496.0 + (double)m;
}

// RN(a / b) for a divisor known on the host: with y = RN(1/b), q = RN(a*y) is a faithful quotient, the fma residual
// r = a - q*b is exact and RN(q + r*y) is the correctly rounded quotient (Markstein) - three instructions instead of
// the ~12-instruction IEEE sequence.  The host checks the precondition (significand of b not all ones).
__device__ __forceinline__ double div_const(double a, double b, double y)
{
    const double q = a * y;
    const double r = fma(-q, b, a);
    return fma(r, y, q);
}

struct glcm_consts {
    double den4, den8, rden4, rden8;  // 4*na*nb, 8*na*nb and their correctly rounded reciprocals
};

// the common denominators of window `win`; false where div_const's precondition does not hold
static inline bool glcm_make_consts(int win, glcm_consts &gc)
{
    const long long na = (long long)win * (win - 1), nb = (long long)(win - 1) * (win - 1);
    gc.den4 = (double)(4 * na * nb);
    gc.den8 = (double)(8 * na * nb);
    gc.rden4 = 1.0 / gc.den4;
    gc.rden8 = 1.0 / gc.den8;
    for (double dv : {gc.den4, gc.den8}) {
        uint64_t b;
        memcpy(&b, &dv, 8);
        if ((b & 0xfffffffffffffull) == 0xfffffffffffffull) return false;
    }
    return true;
}

// the float64 part of the finish: num_c / num_d are the exact contrast and dissimilarity numerators S * nb + S' * na,
// hq0 / hq1 the two groups' homogeneity sums (2^-52 fixed point), sq0 / sq1 their sqrt(A_a) + sqrt(A_b)
__device__ __forceinline__ void glcm_finish_f64(double num_c, double num_d, double hq0, double hq1, double sq0, double sq1, double dna,
                                                double dnb, double r0, double r1, double r2, double r3, size_t o, const glcm_out &out,
                                                const glcm_consts &gc)
{
    if (out.p[0]) out.p[0][o] = (float)div_const(num_c, gc.den4, gc.rden4);
    if (out.p[1]) out.p[1][o] = (float)div_const(num_d, gc.den4, gc.rden4);
    if (out.p[2]) {
        const double t1 = hq1 * dna;
        const double num = fma(hq0, dnb, t1);
        out.p[2][o] = (float)(div_const(num, gc.den4, gc.rden4) * (1.0 / 4503599627370496.0));
    }
    if (out.p[3]) {
        const double t1 = sq1 * dna;
        const double num = fma(sq0, dnb, t1);
        out.p[3][o] = (float)div_const(num, gc.den8, gc.rden8);
    }
    if (out.p[4]) out.p[4][o] = (float)((((r0 + r1) + r2) + r3) * 0.25);
}

// the finish with the two groups' homogeneity sums (2^-52 fixed point) already converted to double
__device__ __forceinline__ void glcm_finish_hq(const glcm_group &g0, const glcm_group &g1, double hq0, double hq1, long long na,
                                               long long nb, double r0, double r1, double r2, double r3, size_t o,
                                               const glcm_out &out, const glcm_consts &gc)
{
    glcm_finish_f64((double)(g0.S2 * nb + g1.S2 * na), (double)(g0.S1 * nb + g1.S1 * na), hq0, hq1, g0.sq, g1.sq, (double)na, (double)nb,
                    r0, r1, r2, r3, o, out, gc);
}

// the register kernels' windows (glcm_fits_int32): S1 / S2 and the numerators in int; the homogeneity sums stay in int64
// (at most 84 terms of 2^52)
struct glcm_group32 {
    int S1, S2;
    long long Hq;
    double sq;
};
__device__ __forceinline__ void glcm_finish32(const glcm_group32 &g0, const glcm_group32 &g1, int na, int nb, double r0, double r1,
                                              double r2, double r3, size_t o, const glcm_out &out, const glcm_consts &gc)
{
    glcm_finish_f64((double)(g0.S2 * nb + g1.S2 * na), (double)(g0.S1 * nb + g1.S1 * na), (double)g0.Hq, (double)g1.Hq, g0.sq, g1.sq,
                    (double)na, (double)nb, r0, r1, r2, r3, o, out, gc);
}

// the launcher of k4_glcm_offsets.hip: `offsets` holds n (dr, dc) entries; def = the four default angles at distance 1,
// finished over their common denominators (gc) like the kernels of k4_glcm.hip
__attribute__((visibility("hidden"))) int glcm_offsets_launch(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int levels, int win,
                                                              int step, const int32_t *offsets, int n, const glcm_out &out, bool def,
                                                              const glcm_consts &gc);
