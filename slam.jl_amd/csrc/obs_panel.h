// obs_panel.h -- what the updates that take up to 8 range-bearing observations share (ekf_iterated.hip, ekf_fej.hip): the block the
// observations travel in and the host code that fills it; the pieces of a front half that do not depend on where the Jacobian was
// evaluated (the gather of P[a, a] and x[a], P[a, a] H', an entry of S; small_front.h factors and solves); the panel kernel that
// forms the PHt rows, W1 and the mean from the Jacobian blocks a front half left in that block; and the enqueue of that kernel and
// the down-date.
#pragma once

#include <vector>

#include "common.h"
#include "../../include/ext/slamhip_iterated.h"
#include "device_math.h"
#include "small_front.h"

constexpr int MO = SLAM_ITERATED_MAXOBS;                   // 8 observations
static_assert(2 * MO == LK, "the observations' rows fill the 16 x 16 front half");
constexpr int NA = 3 + 2 * MO;                             // 19: the states H touches
constexpr int HB = 10;                                     // one observation's Jacobian blocks: Hv (2 x 3, row-major), Hf (2 x 2)
// the block in Smat, in doubles: z[16], R[4] (column-major), idf as int32[8], then -- written by the solve kernel -- Hv | Hf of
// the last iteration, [8][10]
constexpr int B_Z = 0, B_R = LK, B_IDF = B_R + 4, B_H = B_IDF + MO / 2, B_IN = B_H;      // B_H + 80 <= 32 x 32, the smallest Smat

// row t of the reduced H (k x na) times a reduced vector u: the row's five non-zeros
__device__ __forceinline__ double h_row_dot(const double* hbo, int o, int q, const double* u) {
    const double* hv = hbo + 3 * q;
    const double* hf = hbo + 6 + 2 * q;
    return __builtin_fma(hf[1], u[4 + 2 * o], __builtin_fma(hf[0], u[3 + 2 * o], __builtin_fma(hv[2], u[2], __builtin_fma(hv[1], u[1], hv[0] * u[0]))));
}

// ---- the front half, one workgroup of 256 on the calling kernel's LDS arrays: k = 2m rows, na = 3 + 2m reduced states -----------------
// the reduced states' indices, z and R from the block; ends on a barrier
__device__ __forceinline__ void obs_tables(const double* __restrict__ blob, int m, int* cols, double* zs, double* Rs) {
    const int tid = threadIdx.x, k = 2 * m, na = 3 + 2 * m;
    const int32_t* __restrict__ idf = reinterpret_cast<const int32_t*>(blob + B_IDF);
    if (tid < NA) cols[tid] = tid < 3 ? tid : (tid < na ? 3 + 2 * (idf[(tid - 3) >> 1] - 1) + ((tid - 3) & 1) : 0);
    if (tid < LK) zs[tid] = tid < k ? blob[B_Z + tid] : 0.0;
    if (tid < 4) Rs[tid] = blob[B_R + tid];
    __syncthreads();
}

// P[a, a] and x[a] through cols[]; visible after the caller's next barrier
template <typename T>
__device__ __forceinline__ void obs_gather(const T* __restrict__ x, const T* __restrict__ P, int ld, const int* cols, int na,
                                           double (*Pa)[NA + 1], double* xa) {
    const int tid = threadIdx.x;
    for (int t = tid; t < na * na; t += 256) {
        const int r = t / na, c = t - r * na;
        Pa[r][c] = (double)sym_at(P, ld, kTileLog2<T>, cols[r], cols[c]);
    }
    if (tid < na) xa[tid] = (double)x[cols[tid]];
}

// P[a, a] H' from the Jacobian blocks hb; visible after the caller's next barrier
__device__ __forceinline__ void obs_paht(const double (*hb)[HB], const double (*Pa)[NA + 1], double (*PaHt)[LP], int k, int na) {
    for (int t = threadIdx.x; t < na * LK; t += 256) {
        const int r = t >> 4, c = t & 15;
        PaHt[r][c] = c < k ? h_row_dot(hb[c >> 1], c >> 1, c & 1, Pa[r]) : 0.0;
    }
}

// S[i][j] = H[i, :] (P[a, a] H')[:, j] + (I (x) R)[i][j]; the identity outside the leading k x k
__device__ __forceinline__ double obs_s_entry(const double (*hb)[HB], const double (*PaHt)[LP], const double* Rs, int k, int i, int j) {
    if (i >= k || j >= k) return i == j ? 1.0 : 0.0;
    const int o = i >> 1, q = i & 1;
    const double* hv = hb[o] + 3 * q;
    const double* hf = hb[o] + 6 + 2 * q;
    double s = __builtin_fma(hf[1], PaHt[4 + 2 * o][j], __builtin_fma(hf[0], PaHt[3 + 2 * o][j],
               __builtin_fma(hv[2], PaHt[2][j], __builtin_fma(hv[1], PaHt[1][j], hv[0] * PaHt[0][j]))));
    if ((i >> 1) == (j >> 1)) s += Rs[(j & 1) * 2 + (i & 1)];
    return s;
}

// One thread per row r of the PANEL (npad rows: the rows >= n are written as zero, the down-date has no row guards), one wave a
// workgroup so that the rows are spread over the CUs.  Consecutive threads read consecutive rows of one column of a column-major
// tile wherever (r, f) lies on or below the diagonal tiles -- the access pattern of the product update's pht_body.  A row reads
// P[r, 0:3] once and the pair P[r, f : f + 2] once per DISTINCT landmark, every load issued before the first use.
constexpr int PANEL_THREADS = 64;

template <typename T>
__global__ __launch_bounds__(PANEL_THREADS) void iterated_panel_kernel(T* __restrict__ x, const T* __restrict__ P, int ld, int n, int npad,
                                                                        const double* __restrict__ blob, int m, const double* __restrict__ Cin,
                                                                        const double* __restrict__ gin, T* __restrict__ W1, int pitchW,
                                                                        const int32_t* __restrict__ status) {
    constexpr int L = kTileLog2<T>;
    __shared__ double Cs[LK * LK], gs[LK], hs[MO * HB];
    __shared__ int fu[MO], slot[MO], nds;
    const bool bad = status[0] != 0;                                      // (uniform)
    if (!bad) {
        for (int t = threadIdx.x; t < LK * LK; t += PANEL_THREADS) Cs[t] = Cin[t];
        if (threadIdx.x < LK) gs[threadIdx.x] = gin[threadIdx.x];
        for (int t = threadIdx.x; t < m * HB; t += PANEL_THREADS) hs[t] = blob[B_H + t];
    }
    if (threadIdx.x == 0) {                                               // the distinct landmarks, in the order of their first mention
        const int32_t* __restrict__ idf = reinterpret_cast<const int32_t*>(blob + B_IDF);
        int nd = 0;
        for (int o = 0; o < MO; ++o) {
            int s = 0;
            if (o < m) {
                const int f = 3 + 2 * (idf[o] - 1);
                for (s = 0; s < nd && fu[s] != f; ++s) {}
                if (s == nd) fu[nd++] = f;
            }
            slot[o] = s;
        }
        for (int s = nd; s < MO; ++s) fu[s] = fu[0];
        nds = nd;
    }
    __syncthreads();
    const int r = blockIdx.x * PANEL_THREADS + threadIdx.x;
    if (r >= npad) return;
    T* __restrict__ w = W1 + (size_t)r * pitchW;
    if (bad || r >= n) {
#pragma unroll
        for (int c = 0; c < LK; ++c) w[c] = (T)0;
        return;
    }
    const int nd = nds;
    const T t0 = P[p_off(ld, L, r, 0)], t1 = P[p_off(ld, L, r, 1)], t2 = P[p_off(ld, L, r, 2)];
    T q0[MO], q1[MO];
#pragma unroll
    for (int s = 0; s < MO; ++s) {
        q0[s] = (T)0;
        q1[s] = (T)0;
        if (s < nd) {
            q0[s] = sym_at(P, ld, L, r, fu[s]);                           // P[r, f]: from row f where (r, f) lies above the diagonal tiles
            q1[s] = sym_at(P, ld, L, r, fu[s] + 1);
        }
    }
    const double xr = (double)x[r];
    const double p0 = (double)t0, p1 = (double)t1, p2 = (double)t2;
    double dxr = 0.0, acc[LK];
#pragma unroll
    for (int c = 0; c < LK; ++c) acc[c] = 0.0;
#pragma unroll
    for (int o = 0; o < MO; ++o) {
        if (o < m) {
            const int s = slot[o];
            T a0 = q0[0], a1 = q1[0];
#pragma unroll
            for (int u = 1; u < MO; ++u) {                                // the landmark's pair, by selects: the registers stay registers
                a0 = s == u ? q0[u] : a0;
                a1 = s == u ? q1[u] : a1;
            }
            const double* hbo = hs + o * HB;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const double* hv = hbo + 3 * q;
                const double* hf = hbo + 6 + 2 * q;
                const double pht = __builtin_fma(hf[1], (double)a1, __builtin_fma(hf[0], (double)a0,
                                   __builtin_fma(hv[2], p2, __builtin_fma(hv[1], p1, hv[0] * p0))));
                const int row = 2 * o + q;
#pragma unroll
                for (int c = 0; c < LK; ++c) acc[c] += pht * Cs[row * LK + c];      // C is upper: zero below the diagonal
                dxr += pht * gs[row];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < LK; ++c) w[c] = (T)acc[c];
    x[r] = (T)(xr + dxr);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// the noise rule of the range-bearing updates
static inline int check_R(const double* R) {
    ARG_CHECK(slam_all_finite(R, 4), "R is not finite");
    ARG_CHECK(R[1] == R[2], "R is not symmetric");
    ARG_CHECK(R[0] > 0.0 && R[0] * R[3] - R[1] * R[2] > 0.0, "R is not positive definite");
    return SLAM_OK;
}

// the block for m checked-finite observations and a checked R; the rule it adds: every idf names a landmark of the state
static inline int obs_block_fill(const slam_ekf* h, const double* zf, const int32_t* idf, int m, const double* R, std::vector<double>& blob) {
    blob.assign(B_IN, 0.0);
    int32_t* words = reinterpret_cast<int32_t*>(blob.data() + B_IDF);
    for (int o = 0; o < MO; ++o) words[o] = 1;
    for (int o = 0; o < m; ++o) {
        ARG_CHECK(idf[o] >= 1 && idf[o] <= h->N, "idf entry out of range (Julia: BoundsError)");
        words[o] = idf[o];
        blob[B_Z + 2 * o] = zf[2 * o];
        blob[B_Z + 2 * o + 1] = zf[2 * o + 1];
    }
    for (int q = 0; q < 4; ++q) blob[B_R + q] = R[q];
    return SLAM_OK;
}

// behind a front half that left C, g, the status word and the Jacobian blocks: the panel, then P -= W1 W1' on its 16 columns
template <typename T>
static int enqueue_obs_panel(slam_ekf* h, int m) {
    {
        KTimer t(h, SLAM_K_W1);
        hipLaunchKernelGGL(iterated_panel_kernel<T>, dim3((h->npad + PANEL_THREADS - 1) / PANEL_THREADS), dim3(PANEL_THREADS), 0, h->stream,
                           (T*)h->x, (const T*)h->P, h->ld, 3 + 2 * h->N, h->npad, (const double*)h->Smat, m, (const double*)h->Cmat,
                           (const double*)h->gvec, (T*)h->W1, 2 * h->kcap, (const int32_t*)h->d_status);
    }
    HIP_TRY(hipGetLastError());
    return launch_downdate(h, LK, h->W1, h->W1, 2 * h->kcap, (const int32_t*)nullptr, 0, LK, nullptr);
}
