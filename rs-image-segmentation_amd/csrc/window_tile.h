// The LDS tile walk of the window operators (K5-K8 in k5_window.hip, K20 in k20_postclass.hip): the XCD-aware block -> tile
// map, tile staging with the border rule, the 12-value row read, the row store and the ring walk.  Written once here;
// k5_window.hip's header comment describes the scheme.
#pragma once
#include <type_traits>

#include "border.h"
#include "common.h"

// The tile geometry (TW x TH output pixels per workgroup, CPT columns x RPT rows per thread, TPAD staged columns either side,
// TSTRIDE, WIN_MAXP) belongs to the file that includes this one and is #defined there BEFORE the include: k5_window.hip states
// the geometry of K5-K8 (its tests read it from that file), k20_postclass.hip its own.
#if !defined(TW) || !defined(TH) || !defined(CPT) || !defined(RPT) || !defined(TPAD) || !defined(TSTRIDE) || !defined(WIN_MAXP)
#error "define the tile geometry (TW, TH, CPT, RPT, TPAD, TSTRIDE, WIN_MAXP) before including window_tile.h"
#endif

struct win_planes {
    const void *in[WIN_MAXP];
    void *out[WIN_MAXP];
};

// XCD-aware block -> tile mapping.  Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share an L2), so a
// row-major tile order puts horizontally adjacent tiles — which share the 128-byte lines their 4-column pads touch — on
// DIFFERENT XCDs, and the tile below 64 workgroups later.  Each XCD gets a contiguous run of tiles instead: neighbours in x
// follow each other on one XCD, and the halo rows of the tile above are still in that XCD's L2.  grid.x = 8 * chunk.
struct tile_map {
    int ntx, nt, chunk;
};
// tile map and grid of a stencil launch over nrows x W output pixels of nplanes planes
struct stencil_launch {
    tile_map tm;
    dim3 grid;
    stencil_launch(int nrows, int W, int nplanes = 1)
    {
        tm.ntx = (W + TW - 1) / TW;
        tm.nt = tm.ntx * ((nrows + TH - 1) / TH);
        tm.chunk = (tm.nt + 7) / 8;
        grid = dim3(8 * tm.chunk, 1, nplanes);
    }
};
__device__ __forceinline__ bool tile_of_block(const tile_map &m, int &x0, int &ty0)
{
    const int t = (int)(blockIdx.x & 7u) * m.chunk + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= m.chunk || t >= m.nt) return false;
    const int ty = t / m.ntx;
    x0 = (t - ty * m.ntx) * TW;
    ty0 = ty * TH;
    return true;
}

// a plane's element type: its 4-element vector in memory and LDS, and the register type the stencils compute in
template <typename E> struct elem;
template <> struct elem<float> { typedef float4 vec; typedef float reg; };
template <> struct elem<uint8_t> { typedef uint32_t vec; typedef int reg; };

// tile[(TH + 2R)][TW + 2 PAD]: tile row r holds input row border(yb - R + r), tile column c input column x0 - PAD + c
// (columns further than R outside the image are never read by the stencil and are left zero).  PAD is TPAD for every
// window up to 9; the wider windows of K20 (R up to 7) stage 8 columns on either side.
template <typename E, int R, int PAD = TPAD>
__device__ __forceinline__ void load_tile(E *__restrict__ tile, const E *__restrict__ x, int Hin, int W, int mode, int x0, int yb)
{
    typedef typename elem<E>::vec V;
    static_assert(R <= PAD && PAD % 4 == 0, "the pad holds the halo and keeps the 4-element slots aligned");
    constexpr int STRIDE = TW + 2 * PAD;
    constexpr int NR = TH + 2 * R, SLOTS = STRIDE / 4;
    const bool vec = (W & 3) == 0 && ((uintptr_t)x & (sizeof(V) - 1)) == 0;
    for (int s = threadIdx.x; s < NR * SLOTS; s += 256) {
        const int r = s / SLOTS, g = s - r * SLOTS;
        const int gc = x0 - PAD + 4 * g;
        const E *row = x + (size_t)border_idx(yb - R + r, Hin, mode) * W;
        V v;
        if (vec && gc >= 0 && gc + 3 < W) {
            v = *reinterpret_cast<const V *>(row + gc);
        } else {
            E e[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int c = gc + q;
                e[q] = (c < -R || c >= W + R) ? (E)0 : row[border_idx(c, W, mode)];
            }
            memcpy(&v, e, sizeof(V));
        }
        *reinterpret_cast<V *>(tile + r * STRIDE + 4 * g) = v;
    }
}

// Tile staging, once for every stencil: the workgroup's tile (false, for the whole workgroup, when the chunked map gives it
// none), the tile with its halo in LDS, and the thread's 4 columns (cx) x RPT rows (ry) of it.
struct tile_pos { int x0, ty0, cx, ry; };
template <typename E, int R, int PAD = TPAD>
__device__ __forceinline__ bool stage_tile(E *__restrict__ tile, const E *__restrict__ x, int Hin, int W, int y0, int mode, const tile_map &tm,
                                           tile_pos &t)
{
    if (!tile_of_block(tm, t.x0, t.ty0)) return false;
    load_tile<E, R, PAD>(tile, x, Hin, W, mode, t.x0, y0 + t.ty0);
    __syncthreads();
    t.cx = (threadIdx.x & 63) * CPT;
    t.ry = (threadIdx.x >> 6) * RPT;
    return true;
}

__device__ __forceinline__ void read12(const float *p, float (&v)[12])
{
    const float4 a = reinterpret_cast<const float4 *>(p)[0], b = reinterpret_cast<const float4 *>(p)[1], c = reinterpret_cast<const float4 *>(p)[2];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
}
__device__ __forceinline__ void read12(const uint8_t *p, int (&v)[12])
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    const uint32_t a = w[0], b = w[1], c = w[2];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        v[q] = (a >> (8 * q)) & 255u;
        v[4 + q] = (b >> (8 * q)) & 255u;
        v[8 + q] = (c >> (8 * q)) & 255u;
    }
}

__device__ __forceinline__ void store4(float *out, int W, int orow, int col, const float (&o)[4], bool vec)
{
    float *p = out + (size_t)orow * W + col;
    if (vec) *reinterpret_cast<float4 *>(p) = make_float4(o[0], o[1], o[2], o[3]);
    else
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (col + q < W) p[q] = o[q];
}
__device__ __forceinline__ void store4(uint8_t *out, int W, int orow, int col, const int (&o)[4], bool vec)
{
    uint8_t *p = out + (size_t)orow * W + col;
    if (vec) *reinterpret_cast<uint32_t *>(p) = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
    else
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (col + q < W) p[q] = (uint8_t)o[q];
}
// the usual ending of a walk: the four results of an output row go to the plane, as one vector where W and the pointer allow
template <typename O> struct row_store {
    O *out; int W; bool vec;
    __device__ __forceinline__ row_store(O *out_, int W_) : out(out_), W(W_), vec((W_ & 3) == 0 && ((uintptr_t)out_ & (4 * sizeof(O) - 1)) == 0) {}
    template <typename V> __device__ __forceinline__ void operator()(int orow, int col, const V (&o)[CPT]) const { store4(out, W, orow, col, o, vec); }
};

// The ring walk, once for every stencil.  The thread reads its RPT + 2R tile rows top to bottom; Op::row turns the K values
// w[0 .. K-1] under a column into that row's horizontal term, kept in a K-deep register ring; from the K-th row on Op::col
// closes one output row from the ring entries e(0) .. e(K-1), top to bottom, and emit(output row, first column, the four
// results) ends it.  A thread whose columns or rows lie outside the plane does nothing.
template <int K, typename Op, typename E, typename Emit>
__device__ __forceinline__ void stencil_walk(const E *tile, const tile_pos &t, int W, int nrows, Emit emit)
{
    constexpr int R = K / 2;
    if (t.x0 + t.cx >= W || t.ty0 + t.ry >= nrows) return;
    typename Op::term ring[K][CPT];
#pragma unroll
    for (int j = 0; j < RPT + 2 * R; j++) {
        typename elem<E>::reg v[12];
        read12(tile + (t.ry + j) * TSTRIDE + t.cx, v);
#pragma unroll
        for (int c = 0; c < CPT; c++) ring[j % K][c] = Op::row(v + (TPAD - R + c));
        if (j >= 2 * R) {
            const int i = j - 2 * R, orow = t.ty0 + t.ry + i;
            if (orow < nrows) {
                typename Op::result o[CPT];
#pragma unroll
                for (int c = 0; c < CPT; c++) o[c] = Op::col([&](int dy) -> const typename Op::term & { return ring[(i + dy) % K][c]; });
                emit(orow, t.x0 + t.cx, o);
            }
        }
    }
}
