// ekf_jc.hip -- joint-compatibility data association (joint compatibility branch and bound) for the EKF: slam_ekf_associate_joint and
// slam_ekf_joint_nis (include/slamhip_jc.h, which states the rule).  The companion library libslamhip_jc.so.
//
// Four launches on the handle's stream, no host round trip between them:
//   1. jc_sweep_kernel   one thread per landmark, every observation: nis as the gating sweep forms it (pair_const / pair_eval of
//                        device_math.h, the functions ekf_gate.hip uses).  A candidate (nis < gate1) is appended to its observation's
//                        list through an INTEGER counter; the list holds N entries per observation, so it cannot overflow.  min_i:
//                        per-workgroup partial minima, no atomics.
//   2. jc_lists_kernel   the small second launch, one workgroup: per observation the SLAM_JC_MAXCAND smallest (nis, j) in order (a
//                        selection that does not depend on the order of arrival), min_i, rem, the table of distinct candidate
//                        landmarks in order of first appearance and every candidate's index into it; the counters are re-armed.
//   3. jc_cross_kernel   the parallel part: one thread per pair (a >= b) of table entries writes the 2 x 2 block
//                        Hv_a Pvv Hv_b' + Hv_a P[v,b] Hf_b' + Hf_a P[a,v] Hv_b' + Hf_a P[a,b] Hf_b' (+ R when a == b) and its mirror into
//                        the cross matrix M (2U x 2U, leading dimension 1024, double).  P[a,b] goes through sym_at entry by entry, so both
//                        orders of the landmark ids and a landmark whose coordinate pair straddles a tile edge need nothing special.
//   4. jc_search_kernel  ONE WAVE.  The search is a dependent chain: every test is a forward substitution of the two new rows through
//                        the Cholesky factor L of the current S_H, whose steps depend on each other, and the tests depend on each
//                        other's outcome.  L (at most 128 rows, packed by columns: 66 KB) and y = inv(L) v live in LDS.  Lane r owns rows
//                        r and r + 64 of the right-hand sides; step c broadcasts x_c from its owner and every lane below subtracts
//                        L[r][c] x_c (column-oriented: no reduction inside the chain; a column's rows are contiguous in LDS).  Five wave
//                        reductions per test then give the Schur complement and the new part of y.  Backtracking drops rows (k--).
// slam_ekf_joint_nis uploads the caller's ids as the table and runs launches 3 and 4, the latter without the thresholds.
#include <cmath>

#include "common.h"
#include "../../include/slamhip_jc.h"
#include "device_math.h"

constexpr int JC_OBS = SLAM_JC_MAXOBS;
constexpr int JC_CAND = SLAM_JC_MAXCAND;
constexpr int JC_U = JC_OBS * JC_CAND;          // distinct candidate landmarks at most
constexpr int JC_LD = 2 * JC_U;                 // leading dimension of the cross matrix
constexpr int JC_ROWS = 2 * JC_OBS;             // rows of L at most
constexpr int JC_LPACK = JC_ROWS * (JC_ROWS + 1) / 2;
constexpr int JC_SWEEP = 256;                   // landmarks per workgroup of the sweep

struct JcOut {                                  // what a call brings back, one copy
    int32_t assoc[JC_OBS];
    double info[8];
    int32_t status, pad;
};

struct JcWork {                                 // device
    double z[2 * JC_OBS];                       // the first three arrays are uploaded in one copy
    double chi2[JC_OBS];
    int32_t table[JC_U];                        // 1-based landmark of table entry u
    double cand_nis[JC_U];
    int32_t cand_j[JC_U];
    int32_t cand_u[JC_U];
    int32_t ncand[JC_OBS];
    int32_t rem[JC_OBS];
    double minv[JC_OBS];
    double zp[2 * JC_U];                        // predicted observation of table entry u (the cross kernel's diagonal threads)
    int32_t cnt[JC_OBS];                        // the sweep's append counters; zero between calls
    int32_t U, truncated;
    JcOut out;
};

struct JcIn {                                   // pinned staging, the layout of JcWork's head
    double z[2 * JC_OBS];
    double chi2[JC_OBS];
    int32_t table[JC_U];
};

struct slam_ekf_jc {
    slam_ekf* h;                                // borrowed
    JcWork* w;
    double* M;                                  // [JC_LD][JC_LD]
    double* list_nis;                           // [JC_OBS][cap]
    int32_t* list_j;                            // [JC_OBS][cap]
    double* part;                               // [JC_OBS][cap / JC_SWEEP] partial minima
    int cap;                                    // landmarks the lists hold per observation (multiple of JC_SWEEP)
    JcIn* h_in;                                 // pinned
    JcOut* h_out;                               // pinned
};

namespace {

template <typename T>
__device__ inline void load_pose(const T* __restrict__ x, const T* __restrict__ P, int ld, int L, double pose[3], double pvv[9]) {
    pose[0] = (double)x[0];
    pose[1] = (double)x[1];
    pose[2] = (double)x[2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) pvv[r * 3 + c] = (double)P[p_off(ld, L, r, c)];      // diagonal tile 0: stored complete
}

// the double of lane `src` (wave-uniform) in every lane: two v_readlane_b32
__device__ __forceinline__ double bcast_lane(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(JC_SWEEP) void jc_sweep_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld, int N,
                                                            const T* __restrict__ side, int side_n, JcWork* __restrict__ w, int nz,
                                                            double R0, double R1, double R2, double R3, double gate1,
                                                            double* __restrict__ list_nis, int32_t* __restrict__ list_j, int cap,
                                                            double* __restrict__ part, int nblk) {
    constexpr int L = kTileLog2<T>;
    __shared__ double zs[2 * JC_OBS];
    __shared__ double wmin[JC_SWEEP / 64][JC_OBS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 2 * nz) zs[tid] = w->z[tid];
    const double R[4] = {R0, R1, R2, R3};
    double pose[3], pvv[9];
    load_pose(x, P, ld, L, pose, pvv);
    const int j0 = blockIdx.x * JC_SWEEP + tid;
    const bool valid = j0 < N;
    const double INF = __builtin_inf();
    PairConst pc = {};
    if (valid) {
        const int f = 3 + 2 * j0;
        const ObsModel om = obs_model(pose[0], pose[1], pose[2], (double)x[f], (double)x[f + 1]);
        double pfv[2][3], pff[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pfv[0][c] = (double)P[p_off(ld, L, f, c)];
            pfv[1][c] = (double)P[p_off(ld, L, f + 1, c)];
        }
        pff[0] = (double)side[j0];
        pff[2] = (double)side[(size_t)side_n + j0];
        pff[3] = (double)side[(size_t)2 * side_n + j0];
        pff[1] = pff[2];
        pc = pair_const(om, pvv, pfv, pff, R);
    }
    __syncthreads();
    for (int i = 0; i < nz; ++i) {
        double m = INF;
        if (valid) {
            double nis, nd;                                                     // (nd: the gating sweep's, unused here)
            pair_eval(pc, zs[2 * i], zs[2 * i + 1], nis, nd);
            if (nis < gate1) {                                                  // (false for a NaN)
                const int e = atomicAdd(&w->cnt[i], 1);                         // e < N <= cap: one append per landmark at most
                list_nis[(size_t)i * cap + e] = nis;
                list_j[(size_t)i * cap + e] = j0 + 1;
            }
            if (nis == nis) m = nis;
        }
        m = wave_min(m);
        if (lane == 0) wmin[wave][i] = m;
    }
    __syncthreads();
    if (tid < nz) {
        double m = wmin[0][tid];
#pragma unroll
        for (int v = 1; v < JC_SWEEP / 64; ++v)
            if (wmin[v][tid] < m) m = wmin[v][tid];
        part[(size_t)tid * nblk + blockIdx.x] = m;
    }
}

// ---- launch 2 ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jc_lists_kernel(JcWork* __restrict__ w, int nz, const double* __restrict__ list_nis,
                                                       const int32_t* __restrict__ list_j, int cap, const double* __restrict__ part,
                                                       int nblk) {
    __shared__ int s_j[JC_U];            // 0: the slot is empty
    __shared__ int s_first[JC_U];
    __shared__ int s_u[JC_U];
    __shared__ int s_nc[JC_OBS];
    __shared__ int s_trunc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double INF = __builtin_inf();
    for (int s = tid; s < JC_U; s += 256) s_j[s] = 0;
    if (tid < JC_OBS) s_nc[tid] = 0;
    if (tid == 0) s_trunc = 0;
    __syncthreads();
    for (int i = wave; i < nz; i += 4) {
        const int c = w->cnt[i];
        double m = INF;
        for (int b = lane; b < nblk; b += 64) {
            const double p = part[(size_t)i * nblk + b];
            if (p < m) m = p;
        }
        m = wave_min(m);
        // the JC_CAND smallest (nis, j) in ascending order: each pass takes the smallest entry above the previous one
        double pn = -INF;
        int pj = 0, kept = 0;
        for (int s = 0; s < JC_CAND; ++s) {
            double bn = INF;
            int bj = 0x7fffffff;
            for (int e = lane; e < c; e += 64) {
                const double n = list_nis[(size_t)i * cap + e];
                const int j = list_j[(size_t)i * cap + e];
                const bool above = n > pn || (n == pn && j > pj);
                if (above && (n < bn || (n == bn && j < bj))) { bn = n; bj = j; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double on = __shfl_xor(bn, off);
                const int oj = __shfl_xor(bj, off);
                if (on < bn || (on == bn && oj < bj)) { bn = on; bj = oj; }
            }
            if (bj == 0x7fffffff) break;                                        // (wave-uniform)
            if (lane == 0) {
                w->cand_nis[i * JC_CAND + s] = bn;
                w->cand_j[i * JC_CAND + s] = bj;
                s_j[i * JC_CAND + s] = bj;
            }
            pn = bn;
            pj = bj;
            ++kept;
        }
        if (lane == 0) {
            w->ncand[i] = kept;
            s_nc[i] = kept;
            w->minv[i] = m;
            w->cnt[i] = 0;                                                       // re-armed for the next call
            if (c > JC_CAND) s_trunc = 1;
        }
    }
    __syncthreads();
    // the table of distinct candidate landmarks, in order of first appearance (observation, then rank)
    for (int s = tid; s < JC_U; s += 256) {
        const int j = s_j[s];
        int f = s;
        if (j)
            for (int t = 0; t < 8 * nz && t < s; ++t)                        // (no early exit: the reads do not wait for each other)
                if (s_j[t] == j && t < f) f = t;
        s_first[s] = f;
    }
    __syncthreads();
    if (wave == 0) {
        int U = 0;
        for (int base = 0; base < JC_U; base += 64) {                          // first appearances, numbered in slot order
            const int s = base + lane;
            const bool first = s_j[s] && s_first[s] == s;
            const unsigned long long mask = __ballot(first);
            if (first) {
                const int u = U + __popcll(mask & ((1ull << lane) - 1ull));
                s_u[s] = u;
                w->table[u] = s_j[s];
            }
            U += __popcll(mask);
        }
        const unsigned long long has = __ballot(lane < nz && s_nc[lane] > 0);   // JC_OBS == 64: one observation per lane
        if (lane < nz) w->rem[lane] = lane < 63 ? __popcll(has >> (lane + 1)) : 0;
        if (lane == 0) {
            w->U = U;
            w->truncated = s_trunc;
        }
    }
    __syncthreads();
    for (int s = tid; s < JC_U; s += 256) w->cand_u[s] = s_j[s] ? s_u[s_first[s]] : 0;
}

// ---- launch 3 ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void jc_cross_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld, JcWork* __restrict__ w,
                                                      int Ufixed, double R0, double R1, double R2, double R3, double* __restrict__ M) {
    constexpr int L = kTileLog2<T>;
    const int U = Ufixed >= 0 ? Ufixed : w->U;
    const int a = blockIdx.y, b = blockIdx.x * 64 + (int)threadIdx.x;
    if (a >= U || b > a) return;
    const int fa = 3 + 2 * (w->table[a] - 1), fb = 3 + 2 * (w->table[b] - 1);
    double pose[3], pvv[9];
    load_pose(x, P, ld, L, pose, pvv);
    const ObsModel oa = obs_model(pose[0], pose[1], pose[2], (double)x[fa], (double)x[fa + 1]);
    const ObsModel ob = obs_model(pose[0], pose[1], pose[2], (double)x[fb], (double)x[fb + 1]);
    double pav[2][3], pbv[2][3], pab[2][2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pav[e][c] = (double)P[p_off(ld, L, fa + e, c)];
            pbv[e][c] = (double)P[p_off(ld, L, fb + e, c)];
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) pab[e][g] = (double)sym_at(P, ld, L, fa + e, fb + g);
    }
    double A[2][3], Ca[2][3], Da[2][2];        // Hv_a Pvv, Hf_a P[a,v], Hf_a P[a,b]
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[r][c] = oa.Hv[r * 3 + 0] * pvv[0 * 3 + c] + oa.Hv[r * 3 + 1] * pvv[1 * 3 + c] + oa.Hv[r * 3 + 2] * pvv[2 * 3 + c];
            Ca[r][c] = oa.Hf[r * 2 + 0] * pav[0][c] + oa.Hf[r * 2 + 1] * pav[1][c];
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) Da[r][g] = oa.Hf[r * 2 + 0] * pab[0][g] + oa.Hf[r * 2 + 1] * pab[1][g];
    }
    double B[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            double s = A[r][0] * ob.Hv[q * 3 + 0] + A[r][1] * ob.Hv[q * 3 + 1] + A[r][2] * ob.Hv[q * 3 + 2];
            double t = 0.0;                                                     // Hv_a P[v,b] Hf_b': P[v_c, fb + e] = pbv[e][c]
#pragma unroll
            for (int e = 0; e < 2; ++e)
                t += (oa.Hv[r * 3 + 0] * pbv[e][0] + oa.Hv[r * 3 + 1] * pbv[e][1] + oa.Hv[r * 3 + 2] * pbv[e][2]) * ob.Hf[q * 2 + e];
            s += t;
            s += Ca[r][0] * ob.Hv[q * 3 + 0] + Ca[r][1] * ob.Hv[q * 3 + 1] + Ca[r][2] * ob.Hv[q * 3 + 2];
            s += Da[r][0] * ob.Hf[q * 2 + 0] + Da[r][1] * ob.Hf[q * 2 + 1];
            B[r][q] = s;
        }
    if (a == b) {
        const double R[4] = {R0, R1, R2, R3};
        B[0][0] += R[0];
        B[1][0] += R[1];
        B[1][1] += R[3];
        B[0][1] = B[1][0];                                                      // one value for an entry and its mirror
        w->zp[2 * a] = oa.zp[0];
        w->zp[2 * a + 1] = oa.zp[1];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            M[(size_t)(2 * a + r) * JC_LD + 2 * b + q] = B[r][q];
            M[(size_t)(2 * b + q) * JC_LD + 2 * a + r] = B[r][q];
        }
}

// ---- launch 4 ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lp_off(int c) { return c * JC_ROWS - c * (c - 1) / 2; }      // column c of the packed factor: rows c ..

// forced != 0 (slam_ekf_joint_nis): observation i is paired with table entry i, no thresholds; a pivot that is not positive: status 1
__global__ __launch_bounds__(64) void jc_search_kernel(JcWork* __restrict__ w, const double* __restrict__ M, int nz, int max_nodes,
                                                       double gate2, int forced) {
    extern __shared__ __attribute__((aligned(16))) double Lp[];                 // [JC_LPACK]
    __shared__ double s_y[JC_ROWS], s_invd[JC_ROWS], s_d[JC_OBS + 1];
    __shared__ double s_z[2 * JC_OBS], s_chi[JC_OBS], s_zp[2 * JC_U];
    __shared__ int s_cu[JC_U], s_nc[JC_OBS], s_rem[JC_OBS];
    __shared__ int s_ci[JC_OBS], s_hyp[JC_OBS], s_best[JC_OBS], s_rowu[JC_OBS];
    __shared__ unsigned char s_used[JC_U];
    const int lane = threadIdx.x;
    const int U = forced ? nz : w->U;
    for (int t = lane; t < 2 * nz; t += 64) s_z[t] = w->z[t];
    for (int t = lane; t < 2 * U; t += 64) s_zp[t] = w->zp[t];
    for (int t = lane; t < JC_U; t += 64) {
        s_cu[t] = forced ? 0 : w->cand_u[t];
        s_used[t] = 0;
    }
    {
        const int t = lane;                                                     // JC_OBS == 64
        s_chi[t] = (!forced && t < nz) ? w->chi2[t] : 0.0;
        s_nc[t] = (!forced && t < nz) ? w->ncand[t] : 0;
        s_rem[t] = (!forced && t < nz) ? w->rem[t] : 0;
        s_ci[t] = 0;
        s_hyp[t] = 0;
        s_best[t] = 0;
    }
    if (lane == 0) s_d[0] = 0.0;
    __syncthreads();

    int k = 0, bestk = 0, tests = 0, exhausted = 0, deepest = 0, status = 0;
    double bestd = 0.0;
    int i = 0;
    for (;;) {
        int u = -1;
        if (forced) {
            if (i == nz) break;
            u = i;
        } else {
            if (i == nz) {
                if (k > bestk) {
                    bestk = k;
                    bestd = s_d[k];
                    s_best[lane] = s_hyp[lane];
                }
            } else {
                const int c = s_ci[i], nc = s_nc[i];
                if (c < nc) {
                    s_ci[i] = c + 1;
                    const int cu = s_cu[i * JC_CAND + c];
                    if (s_used[cu]) continue;
                    if (tests == max_nodes) {
                        exhausted = 1;
                        break;
                    }
                    u = cu;
                } else if (c == nc) {
                    s_ci[i] = nc + 1;
                    if (k + s_rem[i] > bestk) {
                        ++i;
                        if (i < nz) s_ci[i] = 0;
                    }
                    continue;
                }
            }
            if (u < 0) {                                                        // level i is done (or a leaf): back to the parent
                --i;
                if (i < 0) break;
                if (s_hyp[i] != 0) {
                    --k;
                    s_used[s_rowu[k]] = 0;
                    s_hyp[i] = 0;
                }
                continue;
            }
        }
        // ---- one joint test: d2(H + (i, u)) at depth k ----
        ++tests;
        if (k + 1 > deepest) deepest = k + 1;
        const int n = 2 * k;
        const double* Mu0 = M + (size_t)(2 * u) * JC_LD;
        const double* Mu1 = Mu0 + JC_LD;
        double b0[2] = {0.0, 0.0}, b1[2] = {0.0, 0.0}, yy[2] = {0.0, 0.0};
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int r = lane + 64 * hh;
            if (r < n) {
                const int col = 2 * s_rowu[r >> 1] + (r & 1);
                b0[hh] = Mu0[col];
                b1[hh] = Mu1[col];
                yy[hh] = s_y[r];
            }
        }
        const double m00 = Mu0[2 * u], m10 = Mu1[2 * u], m11 = Mu1[2 * u + 1];
        // the chain: x_c = b_c / L_cc from the lane that owns row c (a v_readlane: c is wave-uniform), then every row below.  The
        // reciprocal diagonals sit in registers (lane r: rows r and r + 64) and column c + 1 is read while column c is applied, so a
        // step waits for no LDS access of its own.
        const double id0 = lane < n ? s_invd[lane] : 0.0, id1 = lane + 64 < n ? s_invd[lane + 64] : 0.0;
        const int n0 = n < 64 ? n : 64;
        {
            double l0 = (0 < n0 && lane > 0 && lane < n) ? Lp[lane] : 0.0;
            double l1 = (0 < n0 && lane + 64 < n) ? Lp[lane + 64] : 0.0;
            for (int c = 0; c < n0; ++c) {
                const double x0 = bcast_lane(b0[0] * id0, c), x1 = bcast_lane(b1[0] * id0, c);
                const double a0 = l0, a1 = l1;
                if (c + 1 < n0) {
                    const double* col = Lp + lp_off(c + 1) - (c + 1);
                    l0 = (lane > c + 1 && lane < n) ? col[lane] : 0.0;
                    l1 = lane + 64 < n ? col[lane + 64] : 0.0;
                }
                if (lane == c) { b0[0] = x0; b1[0] = x1; }
                b0[0] -= a0 * x0;                                               // (a0 is 0 for the rows at and above c and beyond n)
                b1[0] -= a0 * x1;
                b0[1] -= a1 * x0;
                b1[1] -= a1 * x1;
            }
        }
        if (n > 64) {
            double l1 = (lane + 64 > 64 && lane + 64 < n) ? (Lp + lp_off(64) - 64)[lane + 64] : 0.0;
            for (int c = 64; c < n; ++c) {
                const double x0 = bcast_lane(b0[1] * id1, c - 64), x1 = bcast_lane(b1[1] * id1, c - 64);
                const double a1 = l1;
                if (c + 1 < n) {
                    const double* col = Lp + lp_off(c + 1) - (c + 1);
                    l1 = (lane + 64 > c + 1 && lane + 64 < n) ? col[lane + 64] : 0.0;
                }
                if (lane + 64 == c) { b0[1] = x0; b1[1] = x1; }
                b0[1] -= a1 * x0;
                b1[1] -= a1 * x1;
            }
        }
        const double s00 = wave_sum(b0[0] * b0[0] + b0[1] * b0[1]);
        const double s10 = wave_sum(b1[0] * b0[0] + b1[1] * b0[1]);
        const double s11 = wave_sum(b1[0] * b1[0] + b1[1] * b1[1]);
        const double dy0 = wave_sum(b0[0] * yy[0] + b0[1] * yy[1]);
        const double dy1 = wave_sum(b1[0] * yy[0] + b1[1] * yy[1]);
        const double p0 = m00 - s00;
        const double l00 = sqrt(p0);
        const double l10 = (m10 - s10) / l00;
        const double p1 = (m11 - s11) - l10 * l10;
        const double l11 = sqrt(p1);
        const bool pd = p0 > 0.0 && p0 < __builtin_inf() && p1 > 0.0 && p1 < __builtin_inf();
        const double v0 = s_z[2 * i] - s_zp[2 * u];
        const double v1 = mpi_to_pi_d(s_z[2 * i + 1] - s_zp[2 * u + 1]);
        const double y0 = (v0 - dy0) / l00;
        const double y1 = ((v1 - dy1) - l10 * y0) / l11;
        const double d2 = s_d[k] + (y0 * y0 + y1 * y1);
        bool ok = pd;
        if (forced) {
            if (!pd) {
                status = 1;
                break;
            }
        } else {
            ok = pd && d2 < s_chi[k];
        }
        if (!ok) continue;
        // descend with the pairing: two new rows of L (row r's entry of column c sits at lp_off(c) + r - c)
        __syncthreads();
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int r = lane + 64 * hh;
            if (r < n) {
                double* col = Lp + lp_off(r) - r;
                col[n] = hh ? b0[1] : b0[0];
                col[n + 1] = hh ? b1[1] : b1[0];
            }
        }
        if (lane == 0) {
            Lp[lp_off(n)] = l00;
            Lp[lp_off(n) + 1] = l10;
            Lp[lp_off(n + 1)] = l11;
            s_invd[n] = 1.0 / l00;
            s_invd[n + 1] = 1.0 / l11;
            s_y[n] = y0;
            s_y[n + 1] = y1;
            s_d[k + 1] = d2;
            s_rowu[k] = u;
            s_used[u] = 1;
            s_hyp[i] = u + 1;
        }
        ++k;
        ++i;
        if (lane == 0 && i < nz) s_ci[i] = 0;
        __syncthreads();
    }
    __syncthreads();
    if (forced) {
        if (lane == 0) {
            w->out.info[0] = (double)k;
            w->out.info[1] = s_d[k];
            w->out.status = status;
        }
        return;
    }
    if (lane < nz) {
        const int bu = s_best[lane];
        w->out.assoc[lane] = bu ? w->table[bu - 1] : (w->minv[lane] > gate2 ? -1 : 0);
    }
    if (lane == 0) {
        w->out.info[0] = (double)bestk;
        w->out.info[1] = bestd;
        w->out.info[2] = (double)tests;
        w->out.info[3] = (double)exhausted;
        w->out.info[4] = (double)w->truncated;
        w->out.info[5] = (double)U;
        w->out.info[6] = (double)deepest;
        w->out.info[7] = 0.0;
        w->out.status = 0;
    }
}

void jc_free(slam_ekf_jc* jc) {
    if (!jc) return;
    if (jc->w) (void)hipFree(jc->w);
    if (jc->M) (void)hipFree(jc->M);
    if (jc->list_nis) (void)hipFree(jc->list_nis);
    if (jc->list_j) (void)hipFree(jc->list_j);
    if (jc->part) (void)hipFree(jc->part);
    if (jc->h_in) (void)hipHostFree(jc->h_in);
    if (jc->h_out) (void)hipHostFree(jc->h_out);
    delete jc;
}

// the candidate lists hold N entries per observation
int jc_ensure_lists(slam_ekf_jc* jc, int N) {
    if (N <= jc->cap) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(jc->h->stream));
    if (jc->list_nis) (void)hipFree(jc->list_nis);
    if (jc->list_j) (void)hipFree(jc->list_j);
    if (jc->part) (void)hipFree(jc->part);
    jc->list_nis = nullptr;
    jc->list_j = nullptr;
    jc->part = nullptr;
    jc->cap = 0;
    const int cap = round_up(N, 4 * JC_SWEEP);
    HIP_TRY(hipMalloc((void**)&jc->list_nis, sizeof(double) * (size_t)JC_OBS * cap));
    HIP_TRY(hipMalloc((void**)&jc->list_j, sizeof(int32_t) * (size_t)JC_OBS * cap));
    HIP_TRY(hipMalloc((void**)&jc->part, sizeof(double) * (size_t)JC_OBS * (cap / JC_SWEEP)));
    jc->cap = cap;
    return SLAM_OK;
}

bool finite4(const double R[4]) { return std::isfinite(R[0]) && std::isfinite(R[1]) && std::isfinite(R[2]) && std::isfinite(R[3]); }

template <typename T>
int jc_launch_cross(slam_ekf_jc* jc, int Umax, int Ufixed, const double R[4]) {
    slam_ekf* h = jc->h;
    if (Umax <= 0) return SLAM_OK;
    hipLaunchKernelGGL(jc_cross_kernel<T>, dim3((Umax + 63) / 64, Umax), dim3(64), 0, h->stream, (const T*)h->x, (const T*)h->P, h->ld, jc->w,
                       Ufixed, R[0], R[1], R[2], R[3], jc->M);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

template <typename T>
int jc_associate(slam_ekf_jc* jc, int nz, const double R[4], double gate1, double gate2, int max_nodes) {
    slam_ekf* h = jc->h;
    const int N = h->N;
    const int nblk = (N + JC_SWEEP - 1) / JC_SWEEP;
    if (N > 0) {
        hipLaunchKernelGGL(jc_sweep_kernel<T>, dim3(nblk), dim3(JC_SWEEP), 0, h->stream, (const T*)h->x, (const T*)h->P, h->ld, N,
                           (const T*)h->Pside, h->npad / 2, jc->w, nz, R[0], R[1], R[2], R[3], gate1, jc->list_nis, jc->list_j, jc->cap,
                           jc->part, nblk);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(jc_lists_kernel, dim3(1), dim3(256), 0, h->stream, jc->w, nz, (const double*)jc->list_nis,
                       (const int32_t*)jc->list_j, jc->cap, (const double*)jc->part, nblk);
    HIP_TRY(hipGetLastError());
    int Umax = nz * JC_CAND;
    if (Umax > N) Umax = N;
    const int rc = jc_launch_cross<T>(jc, Umax, -1, R);
    if (rc) return rc;
    hipLaunchKernelGGL(jc_search_kernel, dim3(1), dim3(64), sizeof(double) * JC_LPACK, h->stream, jc->w, (const double*)jc->M, nz,
                       max_nodes, gate2, 0);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int jc_fetch(slam_ekf_jc* jc) {
    HIP_TRY(hipMemcpyAsync(jc->h_out, &jc->w->out, sizeof(JcOut), hipMemcpyDeviceToHost, jc->h->stream));
    HIP_TRY(hipStreamSynchronize(jc->h->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_ekf_jc_create(slam_ekf_jc_t* out, slam_ekf_t h) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr && h != nullptr, "null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&jc_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(sizeof(double) * JC_LPACK)));
    slam_ekf_jc* jc = new slam_ekf_jc();
    memset(jc, 0, sizeof(*jc));
    jc->h = h;
    hipError_t e = hipMalloc((void**)&jc->w, sizeof(JcWork));
    if (e == hipSuccess) e = hipMemsetAsync(jc->w, 0, sizeof(JcWork), h->stream);
    if (e == hipSuccess) e = hipMalloc((void**)&jc->M, sizeof(double) * (size_t)JC_LD * JC_LD);
    if (e == hipSuccess) e = hipHostMalloc((void**)&jc->h_in, sizeof(JcIn), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&jc->h_out, sizeof(JcOut), hipHostMallocDefault);
    if (e != hipSuccess) {
        slam_set_error("slam_ekf_jc_create: %s", hipGetErrorString(e));
        jc_free(jc);
        return e == hipErrorOutOfMemory ? SLAM_E_NOMEM : SLAM_E_HIP;
    }
    *out = jc;
    return SLAM_OK;
}

extern "C" int slam_ekf_jc_destroy(slam_ekf_jc_t jc) {
    ARG_CHECK(jc != nullptr, "null workspace");
    if (jc->h) {
        (void)hipSetDevice(jc->h->device);
        (void)hipStreamSynchronize(jc->h->stream);
    }
    jc_free(jc);
    return SLAM_OK;
}

extern "C" int slam_ekf_associate_joint(slam_ekf_jc_t jc, const double* z, int nz, const double R[4], double gate1, double gate2,
                                        const double* chi2, int64_t max_nodes, int32_t* assoc, double info[8]) {
    SLAM_RANGE();
    ARG_CHECK(jc != nullptr && R != nullptr && info != nullptr, "null argument");
    ARG_CHECK(nz >= 0 && nz <= SLAM_JC_MAXOBS, "nz outside 0 .. SLAM_JC_MAXOBS");
    ARG_CHECK(nz == 0 || (z != nullptr && chi2 != nullptr && assoc != nullptr), "null argument");
    ARG_CHECK(finite4(R), "R is not finite");
    ARG_CHECK(std::isfinite(gate1) && std::isfinite(gate2), "a gate is not finite");
    for (int k = 0; k < nz; ++k) ARG_CHECK(std::isfinite(chi2[k]), "a chi2 entry is not finite");
    ARG_CHECK(max_nodes >= 1 && max_nodes <= SLAM_JC_NODE_CAP, "max_nodes outside 1 .. SLAM_JC_NODE_CAP");
    slam_ekf* h = jc->h;
    HIP_TRY(hipSetDevice(h->device));
    int rc = jc_ensure_lists(jc, h->N);
    if (rc) return rc;
    if (nz > 0) {
        memcpy(jc->h_in->z, z, sizeof(double) * 2 * nz);
        memcpy(jc->h_in->chi2, chi2, sizeof(double) * nz);
        HIP_TRY(hipMemcpyAsync(jc->w, jc->h_in, sizeof(double) * 3 * JC_OBS, hipMemcpyHostToDevice, h->stream));
    }
    rc = h->dtype == SLAM_F32 ? jc_associate<float>(jc, nz, R, gate1, gate2, (int)max_nodes)
                              : jc_associate<double>(jc, nz, R, gate1, gate2, (int)max_nodes);
    if (rc) return rc;
    if ((rc = jc_fetch(jc))) return rc;
    for (int i = 0; i < nz; ++i) assoc[i] = jc->h_out->assoc[i];
    for (int k = 0; k < 8; ++k) info[k] = jc->h_out->info[k];
    return SLAM_OK;
}

extern "C" int slam_ekf_joint_nis(slam_ekf_jc_t jc, const double* z, const int32_t* idf, int m, const double R[4], double* d2) {
    SLAM_RANGE();
    ARG_CHECK(jc != nullptr && z != nullptr && idf != nullptr && R != nullptr && d2 != nullptr, "null argument");
    ARG_CHECK(m >= 1 && m <= SLAM_JC_MAXOBS, "m outside 1 .. SLAM_JC_MAXOBS");
    ARG_CHECK(finite4(R), "R is not finite");
    slam_ekf* h = jc->h;
    for (int i = 0; i < m; ++i) {
        ARG_CHECK(idf[i] >= 1 && idf[i] <= h->N, "landmark id out of range");
        for (int t = 0; t < i; ++t) ARG_CHECK(idf[t] != idf[i], "duplicate landmark id");
    }
    HIP_TRY(hipSetDevice(h->device));
    memcpy(jc->h_in->z, z, sizeof(double) * 2 * m);
    for (int i = 0; i < m; ++i) jc->h_in->table[i] = idf[i];
    HIP_TRY(hipMemcpyAsync(jc->w, jc->h_in, sizeof(JcIn), hipMemcpyHostToDevice, h->stream));
    int rc = h->dtype == SLAM_F32 ? jc_launch_cross<float>(jc, m, m, R) : jc_launch_cross<double>(jc, m, m, R);
    if (rc) return rc;
    hipLaunchKernelGGL(jc_search_kernel, dim3(1), dim3(64), sizeof(double) * JC_LPACK, h->stream, jc->w, (const double*)jc->M, m, 1, 0.0, 1);
    HIP_TRY(hipGetLastError());
    if ((rc = jc_fetch(jc))) return rc;
    if (jc->h_out->status) {
        slam_set_error("joint_nis: the joint innovation covariance is not positive definite (pivot %d)", (int)jc->h_out->info[0]);
        return SLAM_E_NOTPD;
    }
    *d2 = jc->h_out->info[1];
    return SLAM_OK;
}
