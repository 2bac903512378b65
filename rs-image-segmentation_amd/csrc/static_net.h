// Compile-time comparator networks for arrays that live in registers: every index is a constant, so a network unrolls into
// straight-line code.  A HOLDER is a type whose static constexpr member `net` has the comparators a[0..n), b[0..n) (a < b in
// value afterwards) and, for the merging networks, `order`: the register indices in ascending order of their values.
#pragma once
#include <utility>

#include <hip/hip_runtime.h>

template <typename F, int... I> __device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void static_for(F &&f)
{
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Sorting network for P elements: Batcher's merge exchange for an arbitrary count (Knuth, TAOCP 5.2.2, Algorithm M) —
// 309 comparators at P = 42, 241 at P = 36 (the power-of-two odd-even merge sort with the padded slots pruned: 327, 268)
template <int P> struct sort_net {
    int a[P * 12], b[P * 12];
    int n;
};
template <int P> constexpr sort_net<P> make_sort_net()
{
    sort_net<P> s{};
    int t = 0;
    while ((1 << t) < P) t++;
    int n = 0;
    for (int p = t > 0 ? 1 << (t - 1) : 0; p > 0; p /= 2) {
        int q = 1 << (t - 1), r = 0, d = p;
        while (d > 0) {
            for (int i = 0; i + d < P; i++)
                if ((i & p) == r) {
                    s.a[n] = i;
                    s.b[n] = i + d;
                    n++;
                }
            d = q - p;
            q /= 2;
            r = p;
        }
    }
    s.n = n;
    return s;
}
template <int P> struct net_holder {
    static constexpr sort_net<P> net = make_sort_net<P>();
};

// Batcher's odd-even (m, n)-merging network (Knuth 5.3.4) on registers [0, M + N): the first run is sorted and laid out in
// the registers first[0..M) (in ascending order of their values), the second is sorted in the registers [M, M + N)
template <int M, int N> struct merge_net {
    int a[(M + N) * 8], b[(M + N) * 8];
    int n;
    int order[M + N];  // register indices in ascending order of their values after the network
};
struct merge_emit {
    int *a, *b, *n;
};
// merges the sorted runs held in registers x[0..m) and y[0..n): comparators appended to e, ascending order to out
constexpr void oem_build(const int *x, int m, const int *y, int n, int *out, merge_emit e)
{
    if (m == 0) { for (int i = 0; i < n; i++) out[i] = y[i]; return; }
    if (n == 0) { for (int i = 0; i < m; i++) out[i] = x[i]; return; }
    if (m == 1 && n == 1) {
        e.a[*e.n] = x[0]; e.b[*e.n] = y[0]; (*e.n)++;
        out[0] = x[0]; out[1] = y[0];
        return;
    }
    int xe[64] = {}, xo[64] = {}, ye[64] = {}, yo[64] = {}, v[128] = {}, w[128] = {};
    int me = 0, mo = 0, ne = 0, no = 0;
    for (int i = 0; i < m; i++) { if (i & 1) xo[mo++] = x[i]; else xe[me++] = x[i]; }
    for (int i = 0; i < n; i++) { if (i & 1) yo[no++] = y[i]; else ye[ne++] = y[i]; }
    oem_build(xe, me, ye, ne, v, e);
    oem_build(xo, mo, yo, no, w, e);
    const int lv = me + ne, lw = mo + no;
    int k = 0;
    out[k++] = v[0];
    for (int i = 0; i < lw; i++) {
        if (i + 1 < lv) {
            e.a[*e.n] = w[i]; e.b[*e.n] = v[i + 1]; (*e.n)++;
            out[k++] = w[i];
            out[k++] = v[i + 1];
        } else {
            out[k++] = w[i];
        }
    }
    for (int i = lw + 1; i < lv; i++) out[k++] = v[i];
}
template <int M, int N> constexpr merge_net<M, N> make_merge_net(const int *first)
{
    merge_net<M, N> s{};
    int y[N] = {};
    for (int i = 0; i < N; i++) y[i] = M + i;
    int n = 0;
    oem_build(first, M, y, N, s.order, merge_emit{s.a, s.b, &n});
    s.n = n;
    return s;
}
// zero-one principle restricted to merging: every pair of sorted 0/1 runs must come out sorted
template <int M, int N> constexpr bool merge_net_ok(const merge_net<M, N> &s, const int *first)
{
    for (int za = 0; za <= M; za++)
        for (int zb = 0; zb <= N; zb++) {
            int r[M + N] = {};
            for (int i = 0; i < M; i++) r[first[i]] = i >= za;
            for (int i = 0; i < N; i++) r[M + i] = i >= zb;
            for (int c = 0; c < s.n; c++) {
                const int lo = r[s.a[c]] < r[s.b[c]] ? r[s.a[c]] : r[s.b[c]], hi = r[s.a[c]] + r[s.b[c]] - lo;
                r[s.a[c]] = lo;
                r[s.b[c]] = hi;
            }
            for (int i = 1; i < M + N; i++)
                if (r[s.order[i - 1]] > r[s.order[i]]) return false;
        }
    return true;
}
// the layout of a run that was sorted in place: register i holds the i-th smallest value
template <int N> struct identity_run {
    int order[N];
};
template <int N> constexpr identity_run<N> make_identity_run()
{
    identity_run<N> s{};
    for (int i = 0; i < N; i++) s.order[i] = i;
    return s;
}
template <int N> struct identity_holder {
    static constexpr identity_run<N> net = make_identity_run<N>();
};
// FIRST: the holder whose `order` describes the first run.  A chain merge_holder<A, B>, merge_holder<A + B, C, merge_holder<A, B>>
// merges three runs in two stages, the second starting from the first's output order.
template <int M, int N, typename FIRST = identity_holder<M>> struct merge_holder {
    static constexpr merge_net<M, N> net = make_merge_net<M, N>(FIRST::net.order);
    static_assert(merge_net_ok(net, FIRST::net.order), "odd-even merging network does not merge");
};

// the order in which a pass visits the registers of a sorted array: as a holder's network left them, or in place
template <typename NET> struct order_of {
    constexpr int operator()(int i) const { return NET::net.order[i]; }
};
struct order_identity {
    constexpr int operator()(int i) const { return i; }
};
