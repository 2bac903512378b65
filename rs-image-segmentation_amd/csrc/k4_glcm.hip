// K4 — GLCM texture windows (contrast, dissimilarity, homogeneity, energy, correlation; mean over the
// angles 0/45/90/135 degrees at distance 1; symmetric, normalised co-occurrence).
//
// Replaces the Python double loop of calculate_glcm_features (reference modules/features/indices.py:
// 283-305: graycomatrix + 5 x graycoprops per window; scikit-image semantics restated in oracle/oracle.c).
//
// The co-occurrence matrix is never formed.  All five properties follow from exact integer
// statistics of the window's pixel pairs (a, b), per angle:
//     np = #pairs, S1 = sum|a-b|, XY = sum a*b, M1 = sum(a+b), M2 = sum(a^2+b^2),  S2 = M2 - 2 XY,
//     Hq = sum round(2^52/(1+(a-b)^2)),
//     A  = sum_ij (G_ij+G_ji)^2 = 2*(np + D) + 4*E2,  D = #{p : a_p == b_p},
//          E2 = sum over runs of equal unordered keys of w*c(c-1)/2, w = 2 on the diagonal else 1
// and the float64 formulas at the end are those of oracle.c (mode 1), so results are bit-identical.
// Angles 0/90 (np = w(w-1)) and 45/135 (np = (w-1)^2) are combined over common denominators, which
// leaves 8 float64 divisions and 4 square roots per window.
//
// Five kernel families; rsseg_glcm_u8 at the end of the file picks one from the geometry.
//   Register-resident (WIN <= 7, levels <= 64): the window lives in 2*WIN registers, 4 pixels per register: pair moments
//   come from v_sad_u8 / v_dot4_u32_u8 on whole rows; the unordered pair keys (13 bits) of TWO angles share a register and go
//   through networks of v_pk_min_u16 / v_pk_max_u16, then a packed run-length pass.  Integer-VALU-bound, not HBM-bound
//   (1 B/px in, 20 B/px out).
//     k4_glcm_thread<WIN,SH>  one thread per window: windows 3 / 5 / 7 at any step, levels <= 32 (SH = 3) or <= 64 (SH = 2).
//     k4_glcm_pair            window 7, step 1, levels <= 32: two horizontally adjacent windows per thread
//                             (RSSEG_GLCM_DENSE=pair).
//     k4_glcm_quad            the same case with a 2 x 2 block of windows per thread: the default dense kernel.
//   LDS histograms (any window size):
//     k4_glcm_wave<SPLIT>     one wave per window, levels <= 32 (the reference's 21x21 / step 21 default).
//     k4_glcm_wg              one workgroup per window, levels <= 64.
//   (65..256 levels: k4_glcm_offsets.hip.)
// The register kernels differ in how many windows share a key and in nothing else; each step they share is defined once:
//   static_net.h   sorting and merging networks built and checked at compile time
//   pk16.h         packed 16-bit arithmetic, the compare-exchange pass (pk_compare_exchange), the run-length pass (pk_runlength)
//   this file      the packed keys and their Hq table reads (glcm_build_keys and its hq_* policies), the pair moments
//                  (row_moments, window_m1m2), the finish from pre-scaled moments (glcm_finish_stats),
//                  the staging of the tables into LDS (glcm_stage_*)
//   k4_glcm.h      the float64 finish, shared with k4_glcm_offsets.hip
#include <mutex>

#include "common.h"
#include "k4_glcm.h"
#include "pk16.h"

__constant__ long long c_glcm_hq[256];
__device__ long long g_glcm_hq2[1024];  // pair sums hq[dA] + hq[dB] at [dB * 32 + dA] (levels <= 32)
// sqrt((double)(2 i)) for every energy sum A = 2 (np + D) + 4 E2 a 7 x 7 window can have: A / 2 = np + D + 2 E2 with np <= 42,
// D <= np and E2 <= 2 * np (np - 1) / 2 (one run of 42 equal keys on the diagonal, weight 2: the constant window, A = 84^2), so
// i <= 42 + 42 + 2 * 1722 = 3528.  Filled on the device by k4_glcm_sqrt_fill with the sqrt the kernels call; padded to a whole
// number of 16-byte pieces per thread of a workgroup, so that the copy into LDS needs no bounds test.
#define GLCM_SQRT_N 3584
static_assert(42 + 42 + 2 * (2 * (42 * 41 / 2)) < GLCM_SQRT_N && GLCM_SQRT_N % 512 == 0, "sqrt table too short for window 7");
__device__ __attribute__((aligned(16))) double g_glcm_sqrt[GLCM_SQRT_N];

// The tables staged into LDS by a workgroup of 256 threads (the caller's __syncthreads() follows).  Unrolled and without a
// bounds test, the loads of all tables a kernel stages are requested back to back: one memory round trip instead of one
// per piece.
__device__ __forceinline__ void glcm_stage_sqrt(double (&sqt)[GLCM_SQRT_N])
{
#pragma unroll
    for (int k = 0; k < GLCM_SQRT_N / 512; k++)
        reinterpret_cast<double2 *>(sqt)[k * 256 + threadIdx.x] = reinterpret_cast<const double2 *>(g_glcm_sqrt)[k * 256 + threadIdx.x];
}
// BACK_TO_BACK: the unrolled form, for a kernel that stages other tables beside this one; otherwise a loop (a kernel with
// this table alone has nothing to request beside it)
template <bool BACK_TO_BACK> __device__ __forceinline__ void glcm_stage_hq2(long long (&hq2)[1024])
{
    if constexpr (BACK_TO_BACK) {
#pragma unroll
        for (int k = 0; k < 4; k++) hq2[k * 256 + threadIdx.x] = g_glcm_hq2[k * 256 + threadIdx.x];
    } else {
        for (int i = threadIdx.x; i < 1024; i += 256) hq2[i] = g_glcm_hq2[i];
    }
}
// the first N entries of the per-difference table: 32 for levels <= 32, all 256 otherwise
template <int N> __device__ __forceinline__ void glcm_stage_hq(long long (&hq)[N])
{
    static_assert(N <= 256, "one entry per thread");
    if (N == 256 || threadIdx.x < N) hq[threadIdx.x] = c_glcm_hq[threadIdx.x];
}

// ---- the steps the register kernels share --------------------------------------------------------------------------
// The window (or the patch of several windows) holds the pixels PRE-SCALED by 2^SH (SH = 3 for levels <= 32, 2 for levels
// <= 64: still one byte), so that the scaled |a-b| gives the byte offset into the Hq table without a shift and all sums are
// exact multiples that are shifted back at the end.

// compiler fence: the N packed rows are redefined (as far as the compiler can tell) here, e.g. at the top of every group
// iteration, so that the two group bodies cannot be hoisted out of the loop or merged (their combined live ranges would
// not fit the register budget)
template <int N> __device__ __forceinline__ void opaque_rows(unsigned (&w)[8][2])
{
#if defined(__HIP_DEVICE_COMPILE__)
    static_for<N>([&](auto I) {
        unsigned &a = w[I][0];
        unsigned &b = w[I][1];
        asm volatile("" : "+v"(a), "+v"(b));
    });
#endif
}

// the pixel positions (row, column 0..7 of the packed rows) of one pair; pad: the entry does not exist for this half
struct gp_pos {
    int rx, cx, ry, cy;
    bool pad;
};
#define GP_PAD_LO 0x0000fffeu
#define GP_PAD_HI 0xfffc0000u

// Hq policies of glcm_build_keys: which table reads a register's packed difference d = dA' | dB' << 16 (primed = pre-scaled)
// takes, and how many of them are left in flight before the sums are pinned (each read holds two registers).  A caller with
// one sum passes it for both halves.
__device__ __forceinline__ void hq_pin(long long &lo, long long &hi)
{
    pin64(lo);
    if (&hi != &lo) pin64(hi);
}
// hq_pair_sum (SH = 3): t is the 32 x 32 table of PAIR sums t[dB][dA] = Hq(dA) + Hq(dB), one read per register, added to lo;
// up to 6 reads in flight
struct hq_pair_sum {
    const long long *t;
    template <int p> __device__ __forceinline__ void add(unsigned d, long long &lo, long long &hi) const
    {
        // byte offset 8 * (dA + 32 * dB) = lo16(d) * 1 + hi16(d) * 32 in one v_dot2_u32_u16
        const unsigned off = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, d), (us2){1, 32}, 0u, false);
        lo += *reinterpret_cast<const long long *>(reinterpret_cast<const char *>(t) + off);
        if constexpr (p % 6 == 5) hq_pin(lo, hi);
    }
};
// hq_per_half: t is the table Hq(d) itself, one read per half (the halves end up in different sums, or SH = 2: the table
// of pair sums would not fit); up to 2 * EVERY reads in flight
template <int SH, int EVERY> struct hq_per_half {
    const long long *t;
    template <int p> __device__ __forceinline__ void add(unsigned d, long long &lo, long long &hi) const
    {
        lo += *reinterpret_cast<const long long *>(reinterpret_cast<const char *>(t) + ((d & 0xffffu) << (3 - SH)));
        hi += *reinterpret_cast<const long long *>(reinterpret_cast<const char *>(t) + ((d >> 16) << (3 - SH)));
        if constexpr (p % EVERY == EVERY - 1) hq_pin(lo, hi);
    }
};

// Builds COUNT packed keys into K[OFF ..) and adds their Hq table reads (pads included: a pad reads Hq(0)) to HqLo / HqHi.
// Entry p carries the pair WHERE(p, 0) in its low half and WHERE(p, 1) in its high half.
// Key = lo' << 8 | hi' | diag (primed = scaled: the low SH bits of a scaled value are zero, so bit 0 is free for the flag
// [a == b]): one v_lshl_or and one v_or on both halves at once.  A pad is an even value above every real key (no diagonal
// flag, equal to nothing).
template <gp_pos (*WHERE)(int, int), int COUNT, int OFF, typename HQ, int NK>
__device__ __forceinline__ void glcm_build_keys(const unsigned (&P)[8][2], unsigned (&K)[NK], HQ hq, long long &HqLo, long long &HqHi)
{
    static_for<COUNT>([&](auto I) {
        constexpr int p = I;
        constexpr gp_pos A = WHERE(p, 0), B = WHERE(p, 1);
        // v_perm_b32: result byte 0 <- low-half pixel, byte 2 <- high-half pixel, bytes 1 and 3 <- 0
        constexpr unsigned selx = (unsigned)(A.cx & 3) | (0x0cu << 8) | ((unsigned)(4 + (B.cx & 3)) << 16) | (0x0cu << 24);
        constexpr unsigned sely = (unsigned)(A.cy & 3) | (0x0cu << 8) | ((unsigned)(4 + (B.cy & 3)) << 16) | (0x0cu << 24);
        const unsigned x = __builtin_amdgcn_perm(P[B.rx][B.cx >> 2], P[A.rx][A.cx >> 2], selx);
        const unsigned y = __builtin_amdgcn_perm(P[B.ry][B.cy >> 2], P[A.ry][A.cy >> 2], sely);
        const unsigned lo = pk_min(x, y), hi = pk_max(x, y);
        const unsigned d = pk_sub(hi, lo);
        const unsigned one = 0x00010001u;
        const unsigned diag = pk_sub_sat(one, d);  // [a == b] in both halves
        unsigned k = ((lo << 8) | hi) | diag;      // each half stays below 2^16: the 32-bit shift does not cross
        if constexpr (A.pad) k = (k & 0xffff0000u) | GP_PAD_LO;
        if constexpr (B.pad) k = (k & 0x0000ffffu) | GP_PAD_HI;
        K[OFF + p] = k;
        pin32(K[OFF + p]);  // materialise the packed key now (short live ranges)
        hq.template add<p>(d, HqLo, HqHi);
    });
}

// sqrt(A_a) + sqrt(A_b), A = 2 (PAIRS + D) + 4 E2, of the two angles packed in E2 / D
template <int PAIRS> __device__ __forceinline__ double glcm_root_sum(unsigned E2, unsigned D)
{
    const long long Aa = 2ll * (PAIRS + (int)(D & 0xffffu)) + 4ll * (long long)(E2 & 0xffffu);
    const long long Ab = 2ll * (PAIRS + (int)(D >> 16)) + 4ll * (long long)(E2 >> 16);
    return sqrt((double)Aa) + sqrt((double)Ab);
}

// pair moments of one angle from whole packed rows: S1 = sum|a-b|, XY = sum ab, M2 = sum a^2+b^2, M1 = sum a+b
template <int WIN, int DR, int DC>
__device__ __forceinline__ void row_moments(const unsigned (&w)[8][2], unsigned &S1, unsigned &XY)
{
    constexpr int NB = DC == 0 ? WIN : WIN - 1;  // bytes taking part per row
    constexpr unsigned KLO = NB >= 4 ? 0xffffffffu : ((1u << (8 * (NB & 3))) - 1u);
    constexpr unsigned KHI = NB <= 4 ? 0u : ((NB >= 8) ? 0xffffffffu : ((1u << (8 * (NB - 4))) - 1u));
    constexpr int R1 = DR > 0 ? WIN - 1 : WIN;
    S1 = XY = 0;
    static_for<R1>([&](auto I) {
        constexpr int r = I;
        const unsigned a0 = w[r][0], a1 = w[r][1], b0 = w[r + DR][0], b1 = w[r + DR][1];
        unsigned Alo, Ahi, Blo, Bhi;
        if constexpr (DC == 1) {         // (c, c+1): A = bytes 0..WIN-2, B = bytes 1..WIN-1
            Alo = a0 & KLO; Ahi = a1 & KHI;
            Blo = __builtin_amdgcn_alignbyte(b1, b0, 1); Bhi = b1 >> 8;
        } else if constexpr (DC == 0) {
            Alo = a0; Ahi = a1; Blo = b0; Bhi = b1;
        } else {                         // (c, c-1): A = bytes 1..WIN-1 of row r, B = bytes 0..WIN-2 of row r+1
            Alo = __builtin_amdgcn_alignbyte(a1, a0, 1); Ahi = a1 >> 8;
            Blo = b0 & KLO; Bhi = b1 & KHI;
        }
        S1 = __builtin_amdgcn_sad_u8(Alo, Blo, S1);
        XY = __builtin_amdgcn_udot4(Alo, Blo, XY, false);
        if constexpr (WIN > 4) {
            S1 = __builtin_amdgcn_sad_u8(Ahi, Bhi, S1);
            XY = __builtin_amdgcn_udot4(Ahi, Bhi, XY, false);
        }
    });
}

// M1 = sum(a+b) and M2 = sum(a^2+b^2) over the pairs of each angle, from sums the four angles share: with T the
// window total, R0/RL the first/last row, C0/CL the first/last column and the corners (L = WIN-1),
//   0 deg   (r,c)-(r,c+1):    2T - C0 - CL
//   90 deg  (r,c)-(r+1,c):    2T - R0 - RL
//   45 deg  (r,c)-(r+1,c+1):  2T - R0 - RL - C0 - CL + w00 + wLL
//   135 deg (r,c)-(r+1,c-1):  2T - R0 - RL - C0 - CL + w0L + wL0
// and the same with squares (a pixel is the first member of a pair unless it lies in the last row/column the angle
// excludes, the second member unless it lies in the first).  m1[] / m2[] are indexed 0, 45, 90, 135 degrees.
template <int WIN> __device__ __forceinline__ void window_m1m2(const unsigned (&w)[8][2], unsigned (&m1)[4], unsigned (&m2)[4])
{
    constexpr int L = WIN - 1;
    unsigned rs[WIN], rq[WIN];
    static_for<WIN>([&](auto I) {
        constexpr int r = I;
        rs[r] = __builtin_amdgcn_sad_u8(w[r][0], 0u, 0u);
        rq[r] = __builtin_amdgcn_udot4(w[r][0], w[r][0], 0u, false);
        if constexpr (WIN > 4) {
            rs[r] = __builtin_amdgcn_sad_u8(w[r][1], 0u, rs[r]);
            rq[r] = __builtin_amdgcn_udot4(w[r][1], w[r][1], rq[r], false);
        }
    });
    unsigned T = 0, T2 = 0;
    static_for<WIN>([&](auto I) { T += rs[I]; T2 += rq[I]; });
    // first / last column gathered into packed registers (rows 0..3, rows 4..)
    constexpr unsigned s0 = 0x0c0c0400u;                                         // byte 0 of both operands
    constexpr unsigned sl = 0x0c0c0000u | ((4u + (L & 3)) << 8) | (unsigned)(L & 3);  // byte L&3 of both operands
    auto column = [&](auto lastc, unsigned &lo, unsigned &hi) {
        constexpr bool LAST = decltype(lastc)::value;
        constexpr int k = LAST ? (L >> 2) : 0;
        constexpr unsigned sel = LAST ? sl : s0;
        // __builtin_amdgcn_perm(hi_src, lo_src, sel): selector bytes 0..3 pick from lo_src, 4..7 from hi_src
        const unsigned p01 = __builtin_amdgcn_perm(w[1 < WIN ? 1 : 0][k], w[0][k], sel);
        const unsigned p23 = WIN > 2 ? __builtin_amdgcn_perm(w[3 < WIN ? 3 : 0][k], w[2 < WIN ? 2 : 0][k], sel) : 0u;
        lo = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
        if constexpr (WIN == 3) lo &= 0x00ffffffu;
        hi = 0u;
        if constexpr (WIN > 4) {
            const unsigned p45 = __builtin_amdgcn_perm(w[5 < WIN ? 5 : 0][k], w[4][k], sel);
            const unsigned p6 = WIN > 6 ? __builtin_amdgcn_perm(0u, w[6 < WIN ? 6 : 0][k], LAST ? (0x0c0c0c00u | (unsigned)(L & 3)) : 0x0c0c0c00u) : 0u;
            hi = __builtin_amdgcn_perm(p6, p45, 0x05040100u);
            if constexpr (WIN == 5) hi &= 0x000000ffu;
        }
    };
    unsigned c0lo, c0hi, cllo, clhi;
    column(std::false_type{}, c0lo, c0hi);
    column(std::true_type{}, cllo, clhi);
    unsigned C0 = __builtin_amdgcn_sad_u8(c0lo, 0u, 0u), CL = __builtin_amdgcn_sad_u8(cllo, 0u, 0u);
    unsigned C0q = __builtin_amdgcn_udot4(c0lo, c0lo, 0u, false), CLq = __builtin_amdgcn_udot4(cllo, cllo, 0u, false);
    if constexpr (WIN > 4) {
        C0 = __builtin_amdgcn_sad_u8(c0hi, 0u, C0);
        CL = __builtin_amdgcn_sad_u8(clhi, 0u, CL);
        C0q = __builtin_amdgcn_udot4(c0hi, c0hi, C0q, false);
        CLq = __builtin_amdgcn_udot4(clhi, clhi, CLq, false);
    }
    const unsigned w00 = c0lo & 0xffu, w0L = cllo & 0xffu;
    const unsigned wL0 = WIN > 4 ? (c0hi >> (8 * (L - 4))) & 0xffu : (c0lo >> (8 * L)) & 0xffu;
    const unsigned wLL = WIN > 4 ? (clhi >> (8 * (L - 4))) & 0xffu : (cllo >> (8 * L)) & 0xffu;
    const unsigned R = rs[0] + rs[L], Rq = rq[0] + rq[L], C = C0 + CL, Cq = C0q + CLq;
    m1[0] = 2 * T - C;
    m1[2] = 2 * T - R;
    m1[1] = 2 * T - R - C + w00 + wLL;
    m1[3] = 2 * T - R - C + w0L + wL0;
    m2[0] = 2 * T2 - Cq;
    m2[2] = 2 * T2 - Rq;
    m2[1] = 2 * T2 - Rq - Cq + w00 * w00 + wLL * wLL;
    m2[3] = 2 * T2 - Rq - Cq + w0L * w0L + wL0 * wL0;
}

// the float64 finish of one window from its pair moments (still pre-scaled: S1 / m1 by 2^SH, XY / m2 by 2^2SH, undone here:
// exact, every term is a multiple; XY in the order 0, 90, 45, 135 degrees, m1 / m2 in the order 0, 45, 90, 135)
template <int WIN, int SH>
__device__ __forceinline__ void glcm_finish_stats(unsigned S1g0, unsigned S1g1, const unsigned (&XY)[4], const unsigned (&m1)[4],
                                                  const unsigned (&m2)[4], long long Hq0, double sq0, long long Hq1, double sq1, size_t o,
                                                  const glcm_out &out, const glcm_consts &gc)
{
    static_assert(WIN <= 7 && SH >= 2 && glcm_fits_int32<WIN, (256 >> SH)>(), "the 32-bit finish needs (2 np (levels - 1))^2 < 2^31");
    constexpr int NA = WIN * (WIN - 1), NB = (WIN - 1) * (WIN - 1);
    const int xy0 = XY[0] >> (2 * SH), xy90 = XY[1] >> (2 * SH), xy45 = XY[2] >> (2 * SH), xy135 = XY[3] >> (2 * SH);
    const int M20 = m2[0] >> (2 * SH), M245 = m2[1] >> (2 * SH), M290 = m2[2] >> (2 * SH), M2135 = m2[3] >> (2 * SH);
    glcm_group32 g0, g1;
    g0.S1 = S1g0 >> SH;
    g0.S2 = (M20 - 2 * xy0) + (M290 - 2 * xy90);
    g0.Hq = Hq0;
    g0.sq = sq0;
    g1.S1 = S1g1 >> SH;
    g1.S2 = (M245 - 2 * xy45) + (M2135 - 2 * xy135);
    g1.Hq = Hq1;
    g1.sq = sq1;
    const double r0 = glcm_corr32(NA, m1[0] >> SH, M20, 2 * xy0), r1 = glcm_corr32(NB, m1[1] >> SH, M245, 2 * xy45);
    const double r2 = glcm_corr32(NA, m1[2] >> SH, M290, 2 * xy90), r3 = glcm_corr32(NB, m1[3] >> SH, M2135, 2 * xy135);
    glcm_finish32(g0, g1, NA, NB, r0, r1, r2, r3, o, out, gc);
}

// ------------------------------------------------------------------------------------------------
// k4_glcm_thread — one thread per window.
// One angle group: G = 0 -> angles 0 (0,1) and 90 (1,0) degrees, G = 1 -> 45 (1,1) and 135 (1,-1).
// Both angles of a group have the same pair count P, so their keys share registers (low / high half).
// ------------------------------------------------------------------------------------------------
// pair p of the group's first (half 0) and second angle (half 1)
template <int WIN, int G> __host__ __device__ constexpr gp_pos gt_where(int p, int half)
{
    if (G == 0) {
        if (half == 0) return gp_pos{p / (WIN - 1), p % (WIN - 1), p / (WIN - 1), p % (WIN - 1) + 1, false};
        return gp_pos{p / WIN, p % WIN, p / WIN + 1, p % WIN, false};
    }
    if (half == 0) return gp_pos{p / (WIN - 1), p % (WIN - 1), p / (WIN - 1) + 1, p % (WIN - 1) + 1, false};
    return gp_pos{p / (WIN - 1), p % (WIN - 1) + 1, p / (WIN - 1) + 1, p % (WIN - 1), false};
}
struct glcm_raw {  // what one angle group leaves behind (S1 / XY still carry the 2^SH pre-scaling)
    unsigned S1, XYa, XYb;
    long long Hq;
    double sq;
};
template <int WIN, int G, int SH>
__device__ __forceinline__ void glcm_group_stats(const unsigned (&w)[8][2], const long long *__restrict__ hq, glcm_raw &g)
{
    constexpr int P = G == 0 ? WIN * (WIN - 1) : (WIN - 1) * (WIN - 1);
    unsigned K[P];
    long long HqA = 0, HqB = 0;
    // every 6 pairs: up to 12 LUT reads (24 registers) in flight, not 2P
    if constexpr (SH == 3) glcm_build_keys<gt_where<WIN, G>, P, 0>(w, K, hq_pair_sum{hq}, HqA, HqB);
    else glcm_build_keys<gt_where<WIN, G>, P, 0>(w, K, hq_per_half<SH, 6>{hq}, HqA, HqB);
    __builtin_amdgcn_sched_barrier(0);  // phase boundaries keep the phases' live ranges from overlapping
    unsigned S1a, XYa, S1b, XYb;
    if constexpr (G == 0) {
        row_moments<WIN, 0, 1>(w, S1a, XYa);
        row_moments<WIN, 1, 0>(w, S1b, XYb);
    } else {
        row_moments<WIN, 1, 1>(w, S1a, XYa);
        row_moments<WIN, 1, -1>(w, S1b, XYb);
    }
    __builtin_amdgcn_sched_barrier(0);
    pk_compare_exchange<net_holder<P>>(K);  // sort both halves at once
    __builtin_amdgcn_sched_barrier(0);
    unsigned E2, D;
    pk_runlength<order_identity>(K, E2, D);
    g.S1 = S1a + S1b;
    g.XYa = XYa;
    g.XYb = XYb;
    g.Hq = HqA + HqB;
    g.sq = glcm_root_sum<P>(E2, D);
}

template <int WIN, int SH>
__global__ __launch_bounds__(256) void k4_glcm_thread(const uint8_t *__restrict__ q, int H, int W, int step, int oh, int ow,
                                                      glcm_out out, glcm_consts gc)
{
    __shared__ long long hq[SH == 3 ? 1024 : 256];
    if constexpr (SH == 3) glcm_stage_hq2<false>(hq);
    else glcm_stage_hq(hq);
    __syncthreads();
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= ow || oy >= oh) return;
    unsigned w[8][2];
    {
        const uint8_t *wp = q + (size_t)(oy * step) * W + (size_t)ox * step;
        static_for<WIN>([&](auto I) {
            constexpr int r = I;
            unsigned lo = 0, hi = 0;
            static_for<WIN>([&](auto J) {
                constexpr int c = J;
                const unsigned b = wp[(size_t)r * W + c];
                if constexpr (c < 4) lo |= b << (8 * c + SH);  // pre-scaled by 2^SH
                else hi |= b << (8 * (c - 4) + SH);
            });
            w[r][0] = lo;
            w[r][1] = hi;
        });
    }
    glcm_raw q0, q1;
#pragma nounroll
    for (int g = 0; g < 2; g++) {
        opaque_rows<WIN>(w);
        if (g == 0) glcm_group_stats<WIN, 0, SH>(w, hq, q0);
        else glcm_group_stats<WIN, 1, SH>(w, hq, q1);
    }
    // M1 / M2 of the four angles (computed after the groups: nothing of it has to stay live across them)
    opaque_rows<WIN>(w);
    unsigned m1[4], m2[4];
    window_m1m2<WIN>(w, m1, m2);
    const unsigned XY[4] = {q0.XYa, q0.XYb, q1.XYa, q1.XYb};
    glcm_finish_stats<WIN, SH>(q0.S1, q1.S1, XY, m1, m2, q0.Hq, q0.sq, q1.Hq, q1.sq, (size_t)oy * ow + ox, out, gc);
}


// ------------------------------------------------------------------------------------------------
// k4_glcm_pair — the dense case (window 7, step 1, levels <= 32) with TWO horizontally adjacent windows per thread.
// Windows x and x+1 share six of their seven columns: 35 of the 42 pair keys of the 0-degree angle, 36 of 42 (90),
// 30 of 36 (45 and 135).  The shared keys are built and sorted ONCE; each window then sorts its own 7 (6) keys and
// merges them into the shared run with Batcher's odd-even (m, n)-merging network (Knuth 5.3.4) before the same
// run-length pass as k4_glcm_thread:   per window 404 compare-exchanges instead of 550, 46 packed keys built instead
// of 78, 46 Hq table reads instead of 78.  The 7 x 8 patch of both windows fits the 14 registers the 7 x 7 window
// already took.  Where an angle has one key fewer than its register partner (35 / 36, 6 / 7) the free half holds a
// pad: an even value above every real key (no diagonal flag, equal to nothing), built from a pixel paired with
// itself so that its table read adds exactly Hq(0) = 2^52, which is subtracted again.
// Same integer statistics, same float64 finish: bit-identical to k4_glcm_thread (and to oracle.c mode 1).
// ------------------------------------------------------------------------------------------------
// pixel positions (patch row, patch column 0..7) of entry p of a key set: SET 0 = shared by both windows,
// 1 = only window A (patch columns 0..6), 2 = only window B (columns 1..7).  half 0 = low 16 bits (angle 0 / 45 degrees),
// half 1 = high 16 bits (90 / 135).
template <int G, int SET> __host__ __device__ constexpr int gp_count() { return G == 0 ? (SET == 0 ? 36 : 7) : (SET == 0 ? 30 : 6); }
template <int G, int SET> __host__ __device__ constexpr gp_pos gp_where(int p, int half)
{
    if (G == 0) {
        if (half == 0) {  // 0 degrees: (r, c)-(r, c+1); pair columns 0 | 1..5 | 6
            if (SET == 0) return p < 35 ? gp_pos{p / 5, 1 + p % 5, p / 5, 2 + p % 5, false} : gp_pos{0, 0, 0, 0, true};
            return SET == 1 ? gp_pos{p, 0, p, 1, false} : gp_pos{p, 6, p, 7, false};
        }
        // 90 degrees: (r, c)-(r+1, c); columns 0 | 1..6 | 7
        if (SET == 0) return gp_pos{p / 6, 1 + p % 6, p / 6 + 1, 1 + p % 6, false};
        if (p >= 6) return gp_pos{0, 0, 0, 0, true};
        return SET == 1 ? gp_pos{p, 0, p + 1, 0, false} : gp_pos{p, 7, p + 1, 7, false};
    }
    if (half == 0) {  // 45 degrees: (r, c)-(r+1, c+1); first columns 0 | 1..5 | 6
        if (SET == 0) return gp_pos{p / 5, 1 + p % 5, p / 5 + 1, 2 + p % 5, false};
        return SET == 1 ? gp_pos{p, 0, p + 1, 1, false} : gp_pos{p, 6, p + 1, 7, false};
    }
    // 135 degrees: (r, c)-(r+1, c-1); first columns 1 | 2..6 | 7
    if (SET == 0) return gp_pos{p / 5, 2 + p % 5, p / 5 + 1, 1 + p % 5, false};
    return SET == 1 ? gp_pos{p, 1, p + 1, 0, false} : gp_pos{p, 7, p + 1, 6, false};
}
template <int G, int SET> __host__ __device__ constexpr int gp_pads()
{
    int n = 0;
    for (int p = 0; p < gp_count<G, SET>(); p++) n += (gp_where<G, SET>(p, 0).pad ? 1 : 0) + (gp_where<G, SET>(p, 1).pad ? 1 : 0);
    return n;
}

// one angle group of both windows: E2 / D per window from the shared sorted run, Hq per window
template <int G>
__device__ __forceinline__ void gp_group(const unsigned (&P)[8][2], const long long *__restrict__ hq, long long &HqA, long long &HqB,
                                         double &sqA, double &sqB)
{
    constexpr int NS = gp_count<G, 0>(), NO = gp_count<G, 1>(), NK = NS + NO;
    constexpr int PAIRS = G == 0 ? 42 : 36;
    using MNET = merge_holder<NS, NO>;
    unsigned KA[NK], KB[NK];
    long long HqS = 0;
    glcm_build_keys<gp_where<G, 0>, NS, 0>(P, KA, hq_pair_sum{hq}, HqS, HqS);
    __builtin_amdgcn_sched_barrier(0);
    pk_compare_exchange<net_holder<NS>>(KA);
    static_for<NS>([&](auto I) { KB[I] = KA[I]; });
    __builtin_amdgcn_sched_barrier(0);
    auto window = [&](auto set_t, unsigned (&K)[NK], long long &Hq, double &sq) {
        constexpr int SET = decltype(set_t)::value;
        long long HqO = 0;
        glcm_build_keys<gp_where<G, SET>, NO, NS>(P, K, hq_pair_sum{hq}, HqO, HqO);
        Hq = HqS + HqO - (long long)(gp_pads<G, 0>() + gp_pads<G, SET>()) * 4503599627370496ll;
        pk_compare_exchange<net_holder<NO>, NS>(K);
        pk_compare_exchange<MNET>(K);
        unsigned E2, D;
        pk_runlength<order_of<MNET>>(K, E2, D);
        sq = glcm_root_sum<PAIRS>(E2, D);
    };
    window(std::integral_constant<int, 1>{}, KA, HqA, sqA);
    __builtin_amdgcn_sched_barrier(0);
    window(std::integral_constant<int, 2>{}, KB, HqB, sqB);
}

// everything of one window that does not involve the key sort: pair moments, M1 / M2, the float64 finish
__device__ __forceinline__ void gp_finish(unsigned (&w)[8][2], long long Hq0, double sq0, long long Hq1, double sq1, size_t o,
                                          const glcm_out &out, const glcm_consts &gc)
{
    constexpr int WIN = 7;
    unsigned S1a, S1b, S1c, S1d, XY[4];
    row_moments<WIN, 0, 1>(w, S1a, XY[0]);
    row_moments<WIN, 1, 0>(w, S1b, XY[1]);
    row_moments<WIN, 1, 1>(w, S1c, XY[2]);
    row_moments<WIN, 1, -1>(w, S1d, XY[3]);
    unsigned m1[4], m2[4];
    window_m1m2<WIN>(w, m1, m2);
    glcm_finish_stats<WIN, 3>(S1a + S1b, S1c + S1d, XY, m1, m2, Hq0, sq0, Hq1, sq1, o, out, gc);
}

__global__ __launch_bounds__(256) void k4_glcm_pair(const uint8_t *__restrict__ q, int H, int W, int oh, int ow, glcm_out out,
                                                    glcm_consts gc)
{
    constexpr int SH = 3;
    __shared__ long long hq[1024];
    glcm_stage_hq2<false>(hq);
    __syncthreads();
    const int ox = 2 * (blockIdx.x * 64 + (threadIdx.x & 63));
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= ow || oy >= oh) return;
    const bool hasB = ox + 1 < ow;  // an odd map width leaves the last thread of a row with one window
    unsigned P[8][2];
    {
        const uint8_t *wp = q + (size_t)oy * W + (size_t)ox;
        static_for<7>([&](auto I) {
            constexpr int r = I;
            unsigned lo = 0, hi = 0;
            static_for<8>([&](auto J) {
                constexpr int c = J;
                const unsigned b = (c < 7 || hasB) ? wp[(size_t)r * W + c] : 0u;
                if constexpr (c < 4) lo |= b << (8 * c + SH);
                else hi |= b << (8 * (c - 4) + SH);
            });
            P[r][0] = lo;
            P[r][1] = hi;
        });
        P[7][0] = P[7][1] = 0;
    }
    long long Hq[2][2];
    double sq[2][2];
#pragma nounroll
    for (int g = 0; g < 2; g++) {
        opaque_rows<7>(P);
        if (g == 0) gp_group<0>(P, hq, Hq[0][0], Hq[1][0], sq[0][0], sq[1][0]);
        else gp_group<1>(P, hq, Hq[0][1], Hq[1][1], sq[0][1], sq[1][1]);
    }
    const size_t o = (size_t)oy * ow + ox;
    unsigned w[8][2];
    opaque_rows<7>(P);
    static_for<7>([&](auto I) {
        w[I][0] = P[I][0];
        w[I][1] = P[I][1] & 0x00ffffffu;
    });
    w[7][0] = w[7][1] = 0;
    gp_finish(w, Hq[0][0], sq[0][0], Hq[0][1], sq[0][1], o, out, gc);
    if (hasB) {
        opaque_rows<7>(P);
        static_for<7>([&](auto I) {
            w[I][0] = __builtin_amdgcn_alignbyte(P[I][1], P[I][0], 1);
            w[I][1] = P[I][1] >> 8;
        });
        gp_finish(w, Hq[1][0], sq[1][0], Hq[1][1], sq[1][1], o + 1, out, gc);
    }
}

// ------------------------------------------------------------------------------------------------
// k4_glcm_quad (r04) — the dense case with a 2 x 2 BLOCK of windows per thread: A = (x, y), B = (x+1, y), C = (x, y+1),
// D = (x+1, y+1) on one 8 x 8 patch (16 registers).  The four windows share, per angle, a CORE of pairs (30 of the 42
// pairs of the 0 / 90 degree angles, 25 of the 36 of 45 / 135), two of them a STRIP of 5 more, and each adds its OWN 7
// (6): the core is built and sorted once per thread, core + strip merged once per two windows, and a window only sorts
// its own keys and merges them in — per window 375 compare-exchanges instead of the pair kernel's 446 and 32 packed keys
// built instead of 46.  The same integer statistics, the same float64 finish (glcm_finish_stats): bit-identical.
//   Finish (r05).  The pair moments of the windows (dx, 0) and (dx, 1) come from per-row sums computed once per column
//   alignment (gq_column_moments), the integer part of the finish runs in 32 bits (k4_glcm.h: glcm_fits_int32) and the four
//   square roots of a window are read from a table of sqrt(2 i) in LDS (g_glcm_sqrt) instead of computed.
//   Packing.  A register carries two angles (low / high half).  For 45 / 135 degrees both halves have the same geometry.
//   For 0 / 90 degrees the geometry of one is the transpose of the other (0: row strips of 5, column strips of 7;
//   90: column strips of 5, row strips of 7), so a register "slot" carries the 0-degree keys of one window and the
//   90-degree keys of its TRANSPOSE partner (A|A, B|C, C|B, D|D): then the merged core + strip array of the top row strip
//   (0 degrees: A, B) and of the left column strip (90 degrees: A, C) is what slots 0 and 1 both start from, and the
//   bottom / right one what slots 2 and 3 start from.  The Hq sums of the sets that are split between windows are read
//   per half from the 32-entry table instead of the table of pair sums.
//   Merging.  Two stages on registers [0, NC + NT + NO): the first merges the sorted runs [0, NC) and [NC, NC + NT), the
//   second merges that run, in the first's output order, with the sorted run [NC + NT, NC + NT + NO).
// ------------------------------------------------------------------------------------------------
// sets of a group: 0 = core, 1 = strip of slots 0 / 1 (0 degrees: top row; 90: left column; 45 / 135: top row),
// 2 = strip of slots 2 / 3 (bottom row; right column), 3 + s = own keys of slot s
template <int G, int SET> __host__ __device__ constexpr int gq_count()
{
    return G == 0 ? (SET == 0 ? 30 : (SET <= 2 ? 5 : 7)) : (SET == 0 ? 25 : (SET <= 2 ? 5 : 6));
}
template <int G, int SET> __host__ __device__ constexpr gp_pos gq_where(int p, int half)
{
    if (G == 0 && half == 0) {   // 0 degrees: (r, c)-(r, c + 1), pair column c in 0..6
        if (SET == 0) return gp_pos{1 + p / 5, 1 + p % 5, 1 + p / 5, 2 + p % 5, false};
        if (SET == 1) return gp_pos{0, 1 + p, 0, 2 + p, false};            // top row strip (A, B)
        if (SET == 2) return gp_pos{7, 1 + p, 7, 2 + p, false};            // bottom row strip (C, D)
        if (SET == 3) return gp_pos{p, 0, p, 1, false};                    // slot 0: A's left column
        if (SET == 4) return gp_pos{p, 6, p, 7, false};                    // slot 1: B's right column
        if (SET == 5) return gp_pos{1 + p, 0, 1 + p, 1, false};            // slot 2: C's left column
        return gp_pos{1 + p, 6, 1 + p, 7, false};                          // slot 3: D's right column
    }
    if (G == 0) {                // 90 degrees: (r, c)-(r + 1, c), pair row r in 0..6
        if (SET == 0) return gp_pos{1 + p / 6, 1 + p % 6, 2 + p / 6, 1 + p % 6, false};
        if (SET == 1) return gp_pos{1 + p, 0, 2 + p, 0, false};            // left column strip (A, C)
        if (SET == 2) return gp_pos{1 + p, 7, 2 + p, 7, false};            // right column strip (B, D)
        if (SET == 3) return gp_pos{0, p, 1, p, false};                    // slot 0: A's top row
        if (SET == 4) return gp_pos{6, p, 7, p, false};                    // slot 1: C's bottom row
        if (SET == 5) return gp_pos{0, 1 + p, 1, 1 + p, false};            // slot 2: B's top row
        return gp_pos{6, 1 + p, 7, 1 + p, false};                          // slot 3: D's bottom row
    }
    // 45 degrees: (r, c)-(r + 1, c + 1); 135 degrees: (r, c + 1)-(r + 1, c); pair row r and pair column c in 0..6
    const int sh = half == 0 ? 0 : 1;
    int r = 0, c = 0;
    if (SET == 0) { r = 1 + p / 5; c = 1 + p % 5; }
    else if (SET == 1) { r = 0; c = 1 + p; }
    else if (SET == 2) { r = 6; c = 1 + p; }
    else if (SET == 3) { r = p; c = 0; }
    else if (SET == 4) { r = p; c = 6; }
    else if (SET == 5) { r = 1 + p; c = 0; }
    else { r = 1 + p; c = 6; }
    return gp_pos{r, c + sh, r + 1, c + 1 - sh, false};
}

// one angle group of the four windows.  ED[s] = D + 2 E2 of slot s (both halves packed: at most 42 + 2 * 1722 per half, so
// A = 2 (np + D) + 4 E2 = 2 (np + ED)); Hq[w] of window w (A, B, C, D)
template <int G>
__device__ __forceinline__ void gq_group(const unsigned (&P)[8][2], const long long *__restrict__ hq2, const long long *__restrict__ hq1,
                                         unsigned (&ED)[4], long long (&Hq)[4])
{
    constexpr int NC = gq_count<G, 0>(), NT = gq_count<G, 1>(), NO = gq_count<G, 3>(), NS = NC + NT, NK = NS + NO;
    using STAGE1 = merge_holder<NC, NT>;
    using STAGE2 = merge_holder<NS, NO, STAGE1>;
    // table reads in flight: 6 pair-sum reads (core, built while few keys are live) or 2 x 2 per-half reads (8 registers:
    // the own-key sets are built at the kernel's register peak)
    const hq_pair_sum whole{hq2};
    const hq_per_half<3, 2> split{hq1};
    unsigned KC[NK], KS[NK], K[NK];    // KC: the sorted core (later core + strip 2, then slot 3 in place); KS: core + strip 1, then slot 1 in place
    long long hqCore = 0, dummy = 0;
    glcm_build_keys<gq_where<G, 0>, NC, 0>(P, KC, whole, hqCore, dummy);
    __builtin_amdgcn_sched_barrier(0);
    pk_compare_exchange<net_holder<NC>>(KC);
    __builtin_amdgcn_sched_barrier(0);
    // Hq of a window = core + its strip halves + its own halves.  Group 0 packs the 0-degree keys of window w with the
    // 90-degree keys of its transpose partner: the low half of slot s belongs to window s, the high half to window
    // part(s) = A, C, B, D; the low half of strip HB to windows 2 HB, 2 HB + 1 (a row strip), the high half to the windows of
    // column HB (A, C / B, D).  Group 1: both halves of everything belong to the slot's own window / row of windows.
    Hq[0] = Hq[1] = Hq[2] = Hq[3] = hqCore;
    // core + strip HB, merged, in S (whose first NC registers hold the sorted core)
    auto add_strip = [&](auto hb_t, unsigned (&S)[NK]) {
        constexpr int HB = decltype(hb_t)::value;
        long long lo = 0, hi = 0;
        glcm_build_keys<gq_where<G, 1 + HB>, NT, NC>(P, S, split, lo, hi);
        Hq[2 * HB] += lo;
        Hq[2 * HB + 1] += lo;
        if constexpr (G == 0) { Hq[HB] += hi; Hq[HB + 2] += hi; }
        else { Hq[2 * HB] += hi; Hq[2 * HB + 1] += hi; }
        pk_compare_exchange<net_holder<NT>, NC>(S);
        pk_compare_exchange<STAGE1>(S);
        __builtin_amdgcn_sched_barrier(0);
    };
    // slot S on the array X whose first NS registers hold core + strip (logical order: STAGE1's)
    auto slot = [&](auto s_t, unsigned (&X)[NK]) {
        constexpr int S = decltype(s_t)::value;
        {
            long long lo = 0, hi = 0;
            glcm_build_keys<gq_where<G, 3 + S>, NO, NS>(P, X, split, lo, hi);
            constexpr int PART = G == 0 ? (S == 1 ? 2 : (S == 2 ? 1 : S)) : S;
            Hq[S] += lo;
            Hq[PART] += hi;
        }
        pk_compare_exchange<net_holder<NO>, NS>(X);
        pk_compare_exchange<STAGE2>(X);
        unsigned E2, D;
        pk_runlength<order_of<STAGE2>>(X, E2, D);
        ED[S] = D + (E2 << 1);
        __builtin_amdgcn_sched_barrier(0);
    };
    // slots 0, 1 from core + strip 1 (a copy of the core: the core itself is needed again); the last user of an array works in place
    static_for<NC>([&](auto I) { KS[I] = KC[I]; });
    add_strip(std::integral_constant<int, 0>{}, KS);
    static_for<NS>([&](auto I) { K[I] = KS[I]; });
    slot(std::integral_constant<int, 0>{}, K);
    slot(std::integral_constant<int, 1>{}, KS);
    add_strip(std::integral_constant<int, 1>{}, KC);
    static_for<NS>([&](auto I) { K[I] = KC[I]; });
    slot(std::integral_constant<int, 2>{}, K);
    slot(std::integral_constant<int, 3>{}, KC);
}

// The pair moments of the two windows (dy = 0, 1) of one column alignment of the 8 x 8 patch: a[r] holds the 7 pixels of patch
// row r that both windows see (byte 7 is zero).  The windows share rows 1..6 and row pairs 1..5, so every per-row quantity
// is computed once over the 8 rows (7 row pairs) and a window adds row 0 or 7 (pair 0 or 6) to the shared part; the two
// shifted forms of a row (bytes 0..5, bytes 1..6) serve the 0, 45 and 135 degree pairs alike.  All sums are exact unsigned
// integers: the same values as row_moments / window_m1m2 give window by window.
struct gq_moments {
    unsigned S1g0, S1g1, XY[4], m1[4], m2[4];   // as glcm_finish_stats takes them
};
__device__ __forceinline__ void gq_column_moments(const unsigned (&a)[8][2], gq_moments (&m)[2])
{
    auto sad2 = [](unsigned xl, unsigned xh, unsigned yl, unsigned yh, unsigned acc) {
        return __builtin_amdgcn_sad_u8(xh, yh, __builtin_amdgcn_sad_u8(xl, yl, acc));
    };
    auto dot2 = [](unsigned xl, unsigned xh, unsigned yl, unsigned yh, unsigned acc) {
        return __builtin_amdgcn_udot4(xh, yh, __builtin_amdgcn_udot4(xl, yl, acc, false), false);
    };
    unsigned Lh[8], Rl[8], Rh[8];    // L = bytes 0..5 (low word: a[r][0] itself), R = bytes 1..6 moved down one byte
    static_for<8>([&](auto I) {
        constexpr int r = I;
        Lh[r] = a[r][1] & 0x0000ffffu;
        Rl[r] = __builtin_amdgcn_alignbyte(a[r][1], a[r][0], 1);
        Rh[r] = a[r][1] >> 8;
    });
    unsigned s0 = 0, s1 = 0, x0 = 0, x90 = 0, x45 = 0, x135 = 0;
    static_for<6>([&](auto I) {      // 0 degrees: rows 1..6
        constexpr int r = 1 + I;
        s0 = sad2(a[r][0], Lh[r], Rl[r], Rh[r], s0);
        x0 = dot2(a[r][0], Lh[r], Rl[r], Rh[r], x0);
    });
    static_for<5>([&](auto I) {      // 90, 45, 135 degrees: row pairs 1..5
        constexpr int r = 1 + I;
        s0 = sad2(a[r][0], a[r][1], a[r + 1][0], a[r + 1][1], s0);
        x90 = dot2(a[r][0], a[r][1], a[r + 1][0], a[r + 1][1], x90);
        s1 = sad2(a[r][0], Lh[r], Rl[r + 1], Rh[r + 1], s1);
        x45 = dot2(a[r][0], Lh[r], Rl[r + 1], Rh[r + 1], x45);
        s1 = sad2(Rl[r], Rh[r], a[r + 1][0], Lh[r + 1], s1);
        x135 = dot2(Rl[r], Rh[r], a[r + 1][0], Lh[r + 1], x135);
    });
    // row totals and squares: rows 2..5 in one chain, rows 0, 1, 6, 7 each (first / last row of a window)
    unsigned in_s = 0, in_q = 0;
    static_for<4>([&](auto I) {
        constexpr int r = 2 + I;
        in_s = sad2(a[r][0], a[r][1], 0u, 0u, in_s);
        in_q = dot2(a[r][0], a[r][1], a[r][0], a[r][1], in_q);
    });
    const unsigned rs0 = sad2(a[0][0], a[0][1], 0u, 0u, 0u), rs1 = sad2(a[1][0], a[1][1], 0u, 0u, 0u);
    const unsigned rs6 = sad2(a[6][0], a[6][1], 0u, 0u, 0u), rs7 = sad2(a[7][0], a[7][1], 0u, 0u, 0u);
    const unsigned rq0 = dot2(a[0][0], a[0][1], a[0][0], a[0][1], 0u), rq1 = dot2(a[1][0], a[1][1], a[1][0], a[1][1], 0u);
    const unsigned rq6 = dot2(a[6][0], a[6][1], a[6][0], a[6][1], 0u), rq7 = dot2(a[7][0], a[7][1], a[7][0], a[7][1], 0u);
    const unsigned mid_s = in_s + rs1 + rs6, mid_q = in_q + rq1 + rq6;
    // columns 0 and 6 over the 8 rows (rows 0..3, rows 4..7); a window leaves out row 7 or row 0
    auto column = [&](auto k_t, unsigned sel, unsigned &lo, unsigned &hi) {
        constexpr int k = decltype(k_t)::value;
        const unsigned p01 = __builtin_amdgcn_perm(a[1][k], a[0][k], sel), p23 = __builtin_amdgcn_perm(a[3][k], a[2][k], sel);
        const unsigned p45 = __builtin_amdgcn_perm(a[5][k], a[4][k], sel), p67 = __builtin_amdgcn_perm(a[7][k], a[6][k], sel);
        lo = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
        hi = __builtin_amdgcn_perm(p67, p45, 0x05040100u);
    };
    unsigned c0lo, c0hi, c6lo, c6hi;
    column(std::integral_constant<int, 0>{}, 0x0c0c0400u, c0lo, c0hi);   // byte 0 of the low words
    column(std::integral_constant<int, 1>{}, 0x0c0c0602u, c6lo, c6hi);   // byte 2 of the high words
    const unsigned Call = sad2(c0lo, c0hi, 0u, 0u, sad2(c6lo, c6hi, 0u, 0u, 0u));
    const unsigned Cqall = dot2(c0lo, c0hi, c0lo, c0hi, dot2(c6lo, c6hi, c6lo, c6hi, 0u));
    static_for<2>([&](auto DY) {
        constexpr int dy = DY, f = dy, l = 6 + dy, x = dy == 0 ? 7 : 0;   // first and last row of the window, the row it leaves out
        constexpr int p = 6 * dy, r = 7 * dy;                             // its own row pair, its own row
        gq_moments &w = m[dy];
        w.S1g0 = sad2(a[p][0], a[p][1], a[p + 1][0], a[p + 1][1], sad2(a[r][0], Lh[r], Rl[r], Rh[r], s0));
        w.XY[0] = dot2(a[r][0], Lh[r], Rl[r], Rh[r], x0);
        w.XY[1] = dot2(a[p][0], a[p][1], a[p + 1][0], a[p + 1][1], x90);
        w.S1g1 = sad2(Rl[p], Rh[p], a[p + 1][0], Lh[p + 1], sad2(a[p][0], Lh[p], Rl[p + 1], Rh[p + 1], s1));
        w.XY[2] = dot2(a[p][0], Lh[p], Rl[p + 1], Rh[p + 1], x45);
        w.XY[3] = dot2(Rl[p], Rh[p], a[p + 1][0], Lh[p + 1], x135);
        auto at = [&](unsigned lo, unsigned hi, int row) { return ((row < 4 ? lo : hi) >> (8 * (row & 3))) & 0xffu; };
        const unsigned w00 = at(c0lo, c0hi, f), w0L = at(c6lo, c6hi, f), wL0 = at(c0lo, c0hi, l), wLL = at(c6lo, c6hi, l);
        const unsigned e0 = at(c0lo, c0hi, x), e6 = at(c6lo, c6hi, x);
        const unsigned T = mid_s + (dy == 0 ? rs0 : rs7), T2 = mid_q + (dy == 0 ? rq0 : rq7);
        const unsigned R = dy == 0 ? rs0 + rs6 : rs1 + rs7, Rq = dy == 0 ? rq0 + rq6 : rq1 + rq7;
        const unsigned C = Call - e0 - e6, Cq = Cqall - e0 * e0 - e6 * e6;
        w.m1[0] = 2 * T - C;
        w.m1[2] = 2 * T - R;
        w.m1[1] = 2 * T - R - C + w00 + wLL;
        w.m1[3] = 2 * T - R - C + w0L + wL0;
        w.m2[0] = 2 * T2 - Cq;
        w.m2[2] = 2 * T2 - Rq;
        w.m2[1] = 2 * T2 - Rq - Cq + w00 * w00 + wLL * wLL;
        w.m2[3] = 2 * T2 - Rq - Cq + w0L * w0L + wL0 * wL0;
    });
}

__global__ __launch_bounds__(256) void k4_glcm_sqrt_fill()
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < GLCM_SQRT_N) g_glcm_sqrt[i] = sqrt((double)(2ll * i));
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k4_glcm_quad(const uint8_t *__restrict__ q, int H, int W, int oh, int ow, glcm_out out,
                                                    glcm_consts gc)
{
    constexpr int SH = 3;
    __shared__ long long hq2[1024];
    __shared__ long long hq1[32];
    // the square roots of the energy sums come from a table (g_glcm_sqrt): four reads per window instead of four float64 sqrt
    __shared__ __attribute__((aligned(16))) double sqt[GLCM_SQRT_N];
    glcm_stage_sqrt(sqt);
    glcm_stage_hq2<true>(hq2);
    glcm_stage_hq(hq1);
    __syncthreads();
    // The window coordinates are needed at the two ends of the kernel only.  Kept in vector registers they (or the thread id
    // they come from) were spilled to scratch memory at the 168-register budget: 3 dwords per thread, +2 B/px of HBM writes in
    // the PMC table.  So they are DERIVED twice from values that cost no vector register in between: the wave's index in
    // the workgroup (uniform: a scalar register) and the lane index (v_mbcnt).
    int wave_s = __builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 6;
    auto coords = [&](int &ox_, int &oy_) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(wave_s));        // opaque: not merged with the other derivation
#endif
        unsigned zero = 0;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(zero));
#endif
        const int lane_ = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
        ox_ = 2 * ((int)blockIdx.x * 64 + lane_);
        oy_ = 2 * ((int)blockIdx.y * 4 + wave_s);
    };
    int ox, oy;
    coords(ox, oy);
    if (ox >= ow || oy >= oh) return;
    bool hasX = ox + 1 < ow, hasY = oy + 1 < oh;   // an odd map width / height leaves the last column / row of threads with fewer windows
    unsigned P[8][2];
    {
        const uint8_t *wp = q + (size_t)oy * W + (size_t)ox;
        static_for<8>([&](auto I) {
            constexpr int r = I;
            unsigned lo = 0, hi = 0;
            static_for<8>([&](auto J) {
                constexpr int c = J;
                const unsigned b = ((c < 7 || hasX) && (r < 7 || hasY)) ? wp[(size_t)r * W + c] : 0u;
                if constexpr (c < 4) lo |= b << (8 * c + SH);
                else hi |= b << (8 * (c - 4) + SH);
            });
            P[r][0] = lo;
            P[r][1] = hi;
        });
    }
    unsigned ED[2][4];
    long long Hq[2][4];
#pragma nounroll
    for (int g = 0; g < 2; g++) {
        opaque_rows<8>(P);
        if (g == 0) gq_group<0>(P, hq2, hq1, ED[0], Hq[0]);
        else gq_group<1>(P, hq2, hq1, ED[1], Hq[1]);
    }
    // A = 2 (np + D) + 4 E2 per window and angle; group 0: window w's 0-degree statistics sit in the low half of slot w,
    // its 90-degree statistics in the high half of its transpose partner's slot (A 0, B 2, C 1, D 3)
    coords(ox, oy);
    hasX = ox + 1 < ow;
    hasY = oy + 1 < oh;
    auto root_sum = [&](int pairs, unsigned ed_lo, unsigned ed_hi) {   // sqrt(A_a) + sqrt(A_b), A = 2 (pairs + ED)
        return sqt[pairs + (int)(ed_lo & 0xffffu)] + sqt[pairs + (int)(ed_hi >> 16)];
    };
    // The windows (dx, 0) and (dx, 1) share their column alignment: one pass of the loop forms the pair moments of both from
    // per-row sums computed once (gq_column_moments) and finishes them.  Window (dx, dy) is slot 2 dy + dx; its transpose
    // partner's slot is 2 dx + dy.
    // RSSEG_GLCM_COUNT_UNROLL (profiles/valu_hist.sh only): the loop unrolled, so that the STATIC instruction histogram of the
    // code object equals the executed one (the shipped kernel keeps the loop rolled: one copy of the finish); the shift is
    // opaque so that the unrolled copies keep the instructions the rolled loop executes
#ifdef RSSEG_GLCM_COUNT_UNROLL
#pragma unroll
#else
#pragma nounroll
#endif
    for (int dx = 0; dx < 2; dx++) {
        if (dx && !hasX) continue;
        int sh = 8 * dx;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(sh));
#endif
        const bool odd = sh != 0;
        unsigned a[8][2];
        opaque_rows<8>(P);
        static_for<8>([&](auto I) {     // patch columns dx .. dx + 6 of every row
            constexpr int r = I;
            a[r][0] = __builtin_amdgcn_alignbit(P[r][1], P[r][0], (unsigned)sh);
            a[r][1] = __builtin_amdgcn_ubfe(P[r][1], (unsigned)sh, 24u);
        });
        gq_moments mo[2];
        gq_column_moments(a, mo);
        static_for<2>([&](auto DY) {
            constexpr int dy = DY;
            if (dy == 0 || hasY) {
                const unsigned e0l = odd ? ED[0][2 * dy + 1] : ED[0][2 * dy], e0h = odd ? ED[0][2 + dy] : ED[0][dy];
                const unsigned e1 = odd ? ED[1][2 * dy + 1] : ED[1][2 * dy];
                const long long h0 = odd ? Hq[0][2 * dy + 1] : Hq[0][2 * dy], h1 = odd ? Hq[1][2 * dy + 1] : Hq[1][2 * dy];
                const double sq0 = root_sum(42, e0l, e0h), sq1 = root_sum(36, e1, e1);
                glcm_finish_stats<7, SH>(mo[dy].S1g0, mo[dy].S1g1, mo[dy].XY, mo[dy].m1, mo[dy].m2, h0, sq0, h1, sq1,
                                (size_t)(oy + dy) * ow + (ox + dx), out, gc);
            }
        });
    }
}

// ---- LDS histogram kernels --------------------------------------------------------------------------------------
// the pairs (r, c)-(r + dr, c + dc) of angle a (0, 45, 90, 135 degrees) in a window: np of them, pw per row, c from c0
struct glcm_angle {
    int dr, dc, c0, pw, np;
};
__device__ __forceinline__ glcm_angle glcm_angle_geometry(int a, int win)
{
    const int dr = a == 0 ? 0 : 1, dc = a == 0 ? 1 : (a == 1 ? 1 : (a == 2 ? 0 : -1));
    const int r1 = dr > 0 ? win - dr : win, c0 = dc < 0 ? -dc : 0, c1 = dc > 0 ? win - dc : win;
    const int pw = c1 - c0;
    return glcm_angle{dr, dc, c0, pw, r1 * pw};
}

// One WAVE per window (levels <= 32, any window size < 256): the four angles' co-occurrence counts live in four private
// 2 KB LDS tables of packed 16-bit counters (a window has fewer than 65536 pairs); no workgroup barrier anywhere — a wave's
// LDS operations execute in order, so its own atomics are complete before its reads.  This is the reference's default
// geometry (window 21, step 21: indices.py:248) — k4_glcm_wg spent most of its 21 us per window in 20 barriers.
// SPLIT: windows above 45 (2048 pairs or more per angle), whose per-angle int64 homogeneity sum would overflow: the lanes'
// partials are reduced split (k4_glcm.h).  Below, the per-angle sums are exact in int64 and only the two-angle group sums
// (which overflow from window 33 on) are formed exactly, on lane 0.
template <bool SPLIT>
__global__ __launch_bounds__(256) void k4_glcm_wave(const uint8_t *__restrict__ q, int H, int W, int levels, int win, int step, int oh,
                                                    int ow, glcm_out out, glcm_consts gc)
{
    __shared__ unsigned hist_all[4][4 * 512];  // [wave][angle][x * 32 + y packed two counters per dword]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long widx = (long long)blockIdx.x * 4 + wave;
    if (widx >= (long long)oh * ow) return;
    const int oy = (int)(widx / ow), ox = (int)(widx - (long long)oy * ow);
    const uint8_t *wp = q + (size_t)(oy * step) * W + (size_t)ox * step;
    unsigned *hist = hist_all[wave];
#pragma unroll
    for (int t = 0; t < 8; t++) reinterpret_cast<uint4 *>(hist)[t * 64 + lane] = make_uint4(0, 0, 0, 0);
    long long sums[4][6];  // per angle: S1 S2 Hq M1 M2 Mx (this lane's share)
    glcm_hq_sum hqs[4];    // SPLIT: per angle Hq split (k4_glcm.h), reduced exactly however large the window
    for (int a = 0; a < 4; a++) {
        const glcm_angle ga = glcm_angle_geometry(a, win);
        const int dr = ga.dr, dc = ga.dc, c0 = ga.c0, pw = ga.pw, P = ga.np;
        int s1 = 0, s2 = 0, m1 = 0, m2 = 0, mx = 0;
        long long hq = 0;
        for (int p = lane; p < P; p += 64) {
            const int r = p / pw, c = c0 + p - r * pw;
            int x = wp[(size_t)r * W + c], y = wp[(size_t)(r + dr) * W + (c + dc)];
            x = x > 31 ? 31 : x;   // the quantiser guarantees < levels; never index outside the table
            y = y > 31 ? 31 : y;
            const int bin = x * 32 + y;
            atomicAdd(&hist[a * 512 + (bin >> 1)], 1u << (16 * (bin & 1)));
            const int d = x > y ? x - y : y - x;
            s1 += d; s2 += d * d; hq += c_glcm_hq[d];
            m1 += x + y; m2 += x * x + y * y; mx += 2 * x * y;
        }
        sums[a][0] = s1; sums[a][1] = s2; sums[a][2] = SPLIT ? 0 : hq; sums[a][3] = m1; sums[a][4] = m2; sums[a][5] = mx;
        if constexpr (SPLIT) hqs[a] = hq_split(hq);  // a lane holds at most ceil(254 * 255 / 64) = 1012 terms of at most 2^52
    }
    long long A[4];
    for (int a = 0; a < 4; a++) {
        const unsigned *h = hist + a * 512;
        long long acc = 0;
        for (int t = lane; t < 1024; t += 64) {
            const int x = t >> 5, y = t & 31, u = y * 32 + x;
            const long long g = (long long)((h[t >> 1] >> (16 * (t & 1))) & 0xffffu) + (long long)((h[u >> 1] >> (16 * (u & 1))) & 0xffffu);
            acc += g * g;
        }
        A[a] = wave_sum(acc);
#pragma unroll
        for (int t = 0; t < 6; t++)
            if (!SPLIT || t != 2) sums[a][t] = wave_sum(sums[a][t]);
        if constexpr (SPLIT) {
            hqs[a].hi = wave_sum(hqs[a].hi);
            hqs[a].lo = wave_sum(hqs[a].lo);
        }
    }
    if (lane == 0) {
        const long long na = (long long)win * (win - 1), nb = (long long)(win - 1) * (win - 1);
        glcm_group g0, g1;
        g0.S1 = sums[0][0] + sums[2][0]; g0.S2 = sums[0][1] + sums[2][1]; g0.Hq = 0;
        g0.sq = sqrt((double)A[0]) + sqrt((double)A[2]);
        g1.S1 = sums[1][0] + sums[3][0]; g1.S2 = sums[1][1] + sums[3][1]; g1.Hq = 0;
        g1.sq = sqrt((double)A[1]) + sqrt((double)A[3]);
        if constexpr (!SPLIT) {
#pragma unroll
            for (int a = 0; a < 4; a++) hqs[a] = hq_split(sums[a][2]);
        }
        const double hq0 = hq_to_double(glcm_hq_sum{hqs[0].hi + hqs[2].hi, hqs[0].lo + hqs[2].lo});
        const double hq1 = hq_to_double(glcm_hq_sum{hqs[1].hi + hqs[3].hi, hqs[1].lo + hqs[3].lo});
        double r[4];
        for (int a = 0; a < 4; a++) r[a] = glcm_corr((a & 1) ? nb : na, sums[a][3], sums[a][4], sums[a][5]);
        glcm_finish_hq(g0, g1, hq0, hq1, na, nb, r[0], r[1], r[2], r[3], (size_t)oy * ow + ox, out, gc);
    }
}

// one workgroup per window; LDS histogram of ordered cells [levels][levels]
__global__ __launch_bounds__(256) void k4_glcm_wg(const uint8_t *__restrict__ q, int H, int W, int levels, int win, int step,
                                                  int oh, int ow, glcm_out out, glcm_consts gc)
{
    extern __shared__ unsigned int hist[];  // levels*levels
    __shared__ long long red[4][9];
    __shared__ long long sst[4][9];
    const int ox = blockIdx.x, oy = blockIdx.y;
    const uint8_t *wp = q + (size_t)(oy * step) * W + (size_t)ox * step;
    const int LL = levels * levels;
    for (int a = 0; a < 4; a++) {
        const glcm_angle ga = glcm_angle_geometry(a, win);
        const int dr = ga.dr, dc = ga.dc, c0 = ga.c0, pw = ga.pw, P = ga.np;
        for (int i = threadIdx.x; i < LL; i += 256) hist[i] = 0;
        __syncthreads();
        long long st[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // np S1 S2 Hq.hi M1 M2 Mx A Hq.lo (Hq split: k4_glcm.h)
        for (int p = threadIdx.x; p < P; p += 256) {
            const int r = p / pw, c = c0 + p % pw;
            const int x = wp[(size_t)r * W + c], y = wp[(size_t)(r + dr) * W + (c + dc)];
            atomicAdd(&hist[x * levels + y], 1u);
            const int d = x > y ? x - y : y - x;
            const long long hq = c_glcm_hq[d];
            st[0] += 1; st[1] += d; st[2] += d * d; st[3] += hq >> GLCM_HQ_SPLIT; st[8] += hq & ((1ll << GLCM_HQ_SPLIT) - 1);
            st[4] += x + y; st[5] += x * x + y * y; st[6] += 2 * x * y;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < LL; i += 256) {
            const int x = i / levels, y = i % levels;
            const long long g = (long long)hist[i] + (long long)hist[y * levels + x];
            st[7] += g * g;
        }
#pragma unroll
        for (int t = 0; t < 9; t++) {
            long long s = wave_sum(st[t]);
            if (lane_id() == 0) red[threadIdx.x >> 6][t] = s;
        }
        __syncthreads();
        if (threadIdx.x < 9) sst[a][threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // sst[a] = np S1 S2 Hq.hi M1 M2 Mx A Hq.lo ; all pixels are < levels, so np depends on the geometry only
        glcm_group g0, g1;
        g0.S1 = sst[0][1] + sst[2][1]; g0.S2 = sst[0][2] + sst[2][2]; g0.Hq = 0;
        g0.sq = sqrt((double)sst[0][7]) + sqrt((double)sst[2][7]);
        g1.S1 = sst[1][1] + sst[3][1]; g1.S2 = sst[1][2] + sst[3][2]; g1.Hq = 0;
        g1.sq = sqrt((double)sst[1][7]) + sqrt((double)sst[3][7]);
        const double hq0 = hq_to_double(glcm_hq_sum{sst[0][3] + sst[2][3], sst[0][8] + sst[2][8]});
        const double hq1 = hq_to_double(glcm_hq_sum{sst[1][3] + sst[3][3], sst[1][8] + sst[3][8]});
        double r[4];
        for (int a = 0; a < 4; a++) r[a] = glcm_corr(sst[a][0], sst[a][4], sst[a][5], sst[a][6]);
        glcm_finish_hq(g0, g1, hq0, hq1, (long long)win * (win - 1), (long long)(win - 1) * (win - 1), r[0], r[1], r[2], r[3],
                    (size_t)oy * ow + ox, out, gc);
    }
}

static bool g_hq_ready[64] = {false};   // per device: the homogeneity tables are in place
static std::mutex g_hq_mu;              // contexts of several threads may arrive together

extern "C" int rsseg_glcm_u8(rsseg_ctx *ctx, const uint8_t *d_q, int H, int W, int levels, int win, int step,
                             float *const *d_props)
{
    if (!ctx) return RSSEG_ERR_INVALID;
    if (!d_q || !d_props || H < 1 || W < 1 || levels < 2 || win < 2 || win > H || win > W || step < 1)
        return rs_fail(ctx, RSSEG_ERR_INVALID, "glcm: bad arguments (H=%d W=%d levels=%d win=%d step=%d)", H, W, levels, win, step);
    if (levels > 256)   // the quantised plane is uint8; NumPy's astype(uint8) of values above 255 is platform-defined
        return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: levels=%d > 256 not supported (the quantised plane is uint8)", levels);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::unique_lock<std::mutex> hq_lock(g_hq_mu);
    if (!g_hq_ready[ctx->device & 63]) {
        long long lut[256];
        for (int d = 0; d < 256; d++) lut[d] = llrint(4503599627370496.0 / (1.0 + (double)d * (double)d));
        HIPCHK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_glcm_hq), lut, sizeof(lut)));
        long long lut2[1024];
        for (int i = 0; i < 1024; i++) lut2[i] = lut[i & 31] + lut[i >> 5];
        HIPCHK(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_glcm_hq2), lut2, sizeof(lut2)));
        // the table of square roots is the device's own sqrt; complete before any other context of this device reads it
        hipLaunchKernelGGL(k4_glcm_sqrt_fill, dim3((GLCM_SQRT_N + 255) / 256), dim3(256), 0, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        g_hq_ready[ctx->device & 63] = true;
    }
    hq_lock.unlock();
    const int oh = (H - win) / step + 1, ow = (W - win) / step + 1;
    glcm_out out;
    for (int i = 0; i < 5; i++) out.p[i] = d_props[i];
    {
        prof_scope ps(ctx, "glcm");
        const dim3 tg((ow + 63) / 64, (oh + 3) / 4);
        glcm_consts gc;
        // div_const needs a divisor whose significand is not all ones: true for these small integers, checked anyway
        if (!glcm_make_consts(win, gc)) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: window size %d not supported", win);
#define GLCM_THREAD(WN)                                                                                                           \
    do {                                                                                                                          \
        if (levels <= 32) hipLaunchKernelGGL((k4_glcm_thread<WN, 3>), tg, dim3(256), 0, ctx->stream, d_q, H, W, step, oh, ow, out, gc); \
        else hipLaunchKernelGGL((k4_glcm_thread<WN, 2>), tg, dim3(256), 0, ctx->stream, d_q, H, W, step, oh, ow, out, gc);          \
    } while (0)
        if (levels > 64) {   // 65..256 levels: the unordered-cell table of k4_glcm_offsets.hip, finished over the same denominators
            static const int32_t def[8] = {0, 1, 1, 1, 1, 0, 1, -1};
            RSCHK(glcm_offsets_launch(ctx, d_q, H, W, levels, win, step, def, 4, out, true, gc));
        } else if (win == 7 && step == 1 && levels <= 32) {
            const char *kv = getenv("RSSEG_GLCM_DENSE");      // "pair": the r02 kernel (two windows per thread), for A/B runs
            if (kv && !strcmp(kv, "pair")) {
                const dim3 pg((ow + 127) / 128, (oh + 3) / 4);   // two adjacent windows per thread
                hipLaunchKernelGGL(k4_glcm_pair, pg, dim3(256), 0, ctx->stream, d_q, H, W, oh, ow, out, gc);
            } else {
                const dim3 pg((ow + 127) / 128, (oh + 7) / 8);   // a 2 x 2 block of windows per thread
                hipLaunchKernelGGL(k4_glcm_quad, pg, dim3(256), 0, ctx->stream, d_q, H, W, oh, ow, out, gc);
            }
        } else if (win == 7) GLCM_THREAD(7);
        else if (win == 5) GLCM_THREAD(5);
        else if (win == 3) GLCM_THREAD(3);
        else {
            if (levels <= 32 && win < 256) {
                const dim3 wg((unsigned)ceil_div64((int64_t)oh * ow, 4));
                if (win <= 45)   // fewer than 2048 pairs per angle: the per-angle int64 homogeneity sums are exact
                    hipLaunchKernelGGL(k4_glcm_wave<false>, wg, dim3(256), 0, ctx->stream, d_q, H, W, levels, win, step, oh, ow, out, gc);
                else
                    hipLaunchKernelGGL(k4_glcm_wave<true>, wg, dim3(256), 0, ctx->stream, d_q, H, W, levels, win, step, oh, ow, out, gc);
            } else if (ow > 2147483647 || oh > 65535) return rs_fail(ctx, RSSEG_ERR_UNSUPPORTED, "glcm: output map too tall for the workgroup-per-window kernel");
            else hipLaunchKernelGGL(k4_glcm_wg, dim3(ow, oh), dim3(256), sizeof(unsigned int) * levels * levels, ctx->stream, d_q, H, W,
                               levels, win, step, oh, ow, out, gc);
        }
    }
    HIPCHK(ctx, hipGetLastError());
    return stream_sync(ctx);
}
