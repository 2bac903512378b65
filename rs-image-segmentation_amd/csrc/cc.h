// Lock-free union-find on a parent plane (Playne & Hawick's atomicMin union), shared by the component filters of K12
// (k12_rules.hip: binary masks, hole filling) and K20 (k20_postclass.hip: the multi-class sieve).  L[i] is pixel i's parent,
// a root is its own parent, and a union hangs the larger root under the smaller, so parents only ever decrease.
#pragma once
#include "common.h"

__device__ __forceinline__ int cc_find(const int *L, int i)
{
    int p = L[i];
    while (p != i) { i = p; p = L[i]; }
    return i;
}
__device__ __forceinline__ void cc_union(int *L, int a, int b)
{
    bool done;
    do {
        a = cc_find(L, a);
        b = cc_find(L, b);
        if (a < b) {
            const int old = atomicMin(&L[b], a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(&L[a], b);
            done = old == a;
            a = old;
        } else
            done = true;
    } while (!done);
}
