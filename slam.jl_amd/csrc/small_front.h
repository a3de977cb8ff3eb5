// small_front.h -- the 16 x 16 front half of the small updates, once: ekf_linear.hip (linear_factor_kernel), ekf_iterated.hip
// (iterated_solve_kernel) and ekf_fej.hip (fej_front_kernel) form their S and v in their own way and then call these pieces, so
// that the three take the same pivots and do the same arithmetic per entry by construction.
//
// One workgroup of 256 on LDS arrays the calling kernel declares.  Thread (i, j) = (tid >> 4, tid & 15) owns entry (i, j) of S in
// the symmetrisation and in the trailing updates of the factorisation; lane r of the first 16 scales row r of a pivot's column and
// owns column r of inv(L).  Rows / columns >= k are the identity, so the chain of pivots stops at k.  Every decision is taken from
// values all threads read from LDS, so it is uniform and every thread reaches every barrier.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

constexpr int LK = 16;                                     // the panel's columns, one chunk of the down-date
constexpr int LP = LK + 1;

// S = (S + S') / 2 in place; the caller has just written its entry M[i][j].  Returns this thread's entry of the result.
__device__ __forceinline__ double small_symmetrise(double (*M)[LP]) {
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    __syncthreads();
    const double sym = (M[i][j] + M[j][i]) * 0.5;
    __syncthreads();
    M[i][j] = sym;
    __syncthreads();
    return sym;
}

// Right-looking Cholesky S = L L' in place (the lower triangle of M).  Returns the index of the failing pivot, or -1; piv is the
// last pivot read (the failing one), lmin the smallest l_cc.  Three barriers a pivot: the chain of k pivots is what a front half
// costs.  dsave (may be null) gets l_cc = sqrt(pivot c) as the chain computes it -- M[c][c] = pivot / l_cc afterwards need not be
// the same number.
__device__ __forceinline__ int small_cholesky(double (*M)[LP], int k, double& piv, double& lmin, double* dsave) {
    const int tid = threadIdx.x, i = tid >> 4, j = tid & 15;
    int fail = -1;
    lmin = INFINITY;
    for (int c = 0; c < k; ++c) {
        piv = M[c][c];
        if (!(piv > 0.0) || !(piv < INFINITY)) { fail = c; break; }
        const double d = sqrt(piv);
        lmin = d < lmin ? d : lmin;
        if (dsave && tid == 0) dsave[c] = d;
        __syncthreads();
        if (tid >= c && tid < LK) M[tid][c] = M[tid][c] / d;
        __syncthreads();
        if (i > c && j > c && j <= i) M[i][j] -= M[i][c] * M[j][c];
        __syncthreads();
    }
    return fail;
}

// inv(L) into Li, y = inv(L) v, g = inv(L)' y.  Returns g[tid] for tid < 16 (0.0 at tid >= k: no term); y is complete, and Li may
// be read, after the caller's next barrier.
__device__ __forceinline__ double small_solve(const double (*M)[LP], double (*Li)[LP], const double* v, double* y, int k) {
    const int tid = threadIdx.x;
    if (tid < k) {       // inv(L): lane c solves L X[:, c] = e_c
        for (int r = 0; r < k; ++r) {
            double s = r == tid ? 1.0 : 0.0;
            for (int q = tid; q < r; ++q) s -= M[r][q] * Li[q][tid];
            Li[r][tid] = r < tid ? 0.0 : s / M[r][r];
        }
    }
    __syncthreads();
    if (tid < k) {       // y = C' v = inv(L) v
        double s = 0.0;
        for (int q = 0; q <= tid; ++q) s += Li[tid][q] * v[q];
        y[tid] = s;
    }
    __syncthreads();
    double s = 0.0;      // g = C y = inv(L)' y
    if (tid < LK)
        for (int q = tid; q < k; ++q) s += Li[q][tid] * y[q];
    return s;
}

// C[i][j] = inv(L)[j][i], zero outside the leading k x k
__device__ __forceinline__ void small_store_c(const double (*Li)[LP], int k, double* Cout) {
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    Cout[threadIdx.x] = (i <= j && j < k) ? Li[j][i] : 0.0;
}
