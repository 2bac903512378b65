// Two unsigned 16-bit lanes per 32-bit register (v_pk_*_u16), and the passes over register arrays of such pairs that
// the texture kernels share: the compare-exchange network and the run-length pass over the sorted keys.
#pragma once
#include "static_net.h"

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_min(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
// max(a - b, 0) on both 16-bit halves (v_pk_sub_u16 with the clamp bit): 1 - d saturates to [d == 0]
__device__ __forceinline__ unsigned pk_sub_sat(unsigned a, unsigned b)
{
    unsigned r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
#endif
    return r;
}
// a * b on both 16-bit halves (v_pk_mul_lo_u16)
__device__ __forceinline__ unsigned pk_mul(unsigned a, unsigned b)
{
    unsigned r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
#endif
    return r;
}
__device__ __forceinline__ unsigned pk_sub(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, (us2)(__builtin_bit_cast(us2, a) - __builtin_bit_cast(us2, b)));
}

// the value is materialised in a vector register here (short live ranges: the compiler cannot defer or rematerialise it)
__device__ __forceinline__ void pin32(unsigned &v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
}
__device__ __forceinline__ void pin64(long long &v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
}

// the comparators of NET::net applied to K[OFF ..), both halves at once
template <typename NET, int OFF = 0, int NK> __device__ __forceinline__ void pk_compare_exchange(unsigned (&K)[NK])
{
    static_for<NET::net.n>([&](auto I) {
        constexpr int ia = OFF + NET::net.a[I], ib = OFF + NET::net.b[I];
        const unsigned ka = K[ia], kb = K[ib];
        K[ia] = pk_min(ka, kb);
        K[ib] = pk_max(ka, kb);
    });
}

// Packed run-length pass over the sorted keys K[ORD(0)], K[ORD(1)], ... (bit 0 of a key: it lies on the diagonal, a == b):
// t = equal-to-previous ? t + w : 0 (w = 2 on the diagonal, else 1); E2 += t; D += diag.  All fields stay far below 2^16,
// so plain 32-bit adds (v_add3_u32) serve both halves.
template <typename ORD, int NK> __device__ __forceinline__ void pk_runlength(const unsigned (&K)[NK], unsigned &E2, unsigned &D)
{
    constexpr ORD ord{};
    const unsigned one = 0x00010001u;
    E2 = 0;
    unsigned t = 0;
    D = K[ord(0)] & one;
    static_for<NK - 1>([&](auto I) {
        constexpr int i = ord(I + 1), j = ord(I);
        const unsigned diag = K[i] & one;
        const unsigned eq = pk_sub_sat(one, K[i] ^ K[j]);   // 1 where the keys are equal, 0 where they differ
        t = pk_mul(t + one + diag, eq);
        E2 += t;
        D += diag;
    });
}
