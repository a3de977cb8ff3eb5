// wave_reduce.h -- full-wave reductions of a double: the xor butterfly over the 64 lanes, offsets 32 down to 1.  Every lane ends
// with the same bits (a + b == b + a), and the order of the additions is the one every fixed-order sum of the library is specified
// with.  Partial trees (a few offsets only), interleaved chains and (value, index) exchanges stay where they are used.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

__device__ __forceinline__ double wave_max(double m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    return m;
}

// by comparison, not fmin: a NaN in another lane never replaces m
__device__ __forceinline__ double wave_min(double m) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(m, off);
        if (o < m) m = o;
    }
    return m;
}
