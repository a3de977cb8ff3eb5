// strip_tail.h -- what the one-launch predicts share behind their column strips (predict_kernel in ekf_strip.hip,
// linear_strip_kernel in ekf_linear.hip, fej_strip_kernel in ekf_fej.hip): every workgroup reads the pose for its part of the
// strip, and the workgroup that arrives LAST at a counter -- after every workgroup has read it -- rewrites P_vv and the pose.
// Nothing is published between workgroups (the strip and the pose block are disjoint), so the arrival is a relaxed atomic
// without fences.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.h"

// true in every thread of the workgroup whose arrival is the grid's last; a barrier on either side of the arrival
__device__ __forceinline__ bool strip_arrive_last(int32_t* __restrict__ arrive) {
    __shared__ int last;
    __syncthreads();                         // every thread of the workgroup has read what the last one rewrites
    if (threadIdx.x == 0)
        last = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    return last;
}

// the counter back at zero for the next launch on the stream
__device__ __forceinline__ void strip_rearm(int32_t* __restrict__ arrive) {
    __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the noise of the bicycle model in the vehicle's block: (Gu Q Gu')[r][c], c <= r, Q column-major as the caller gave it
__device__ __forceinline__ void strip_gu_q_gut(const double Gu[3][2], double Q0, double Q1, double Q2, double Q3, double add[3][3]) {
    const double Q[2][2] = {{Q0, Q2}, {Q1, Q3}};
    double GQ[3][2];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 2; ++c) GQ[r][c] = Gu[r][0] * Q[0][c] + Gu[r][1] * Q[1][c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c <= r; ++c) add[r][c] = GQ[r][0] * Gu[c][0] + GQ[r][1] * Gu[c][1];
}

// P_vv <- G P_vv G' + add by ONE thread: the lower triangle, each entry formed once, converted once and stored with its mirror
// ((r, c) and (c, r) formed separately round differently).  add is read at c <= r.
template <typename T>
__device__ __forceinline__ void strip_rewrite_pvv(T* __restrict__ P, int ld, int tlog, const double G[3][3], const double add[3][3]) {
    double Pvv[3][3], GP[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Pvv[r][c] = (double)P[p_off(ld, tlog, r, c)];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) GP[r][c] = G[r][0] * Pvv[0][c] + G[r][1] * Pvv[1][c] + G[r][2] * Pvv[2][c];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c <= r; ++c) {
            const T val = (T)((GP[r][0] * G[c][0] + GP[r][1] * G[c][1] + GP[r][2] * G[c][2]) + add[r][c]);
            P[p_off(ld, tlog, r, c)] = val;
            P[p_off(ld, tlog, c, r)] = val;
        }
}
