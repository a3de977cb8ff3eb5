// ekf_wide.hip -- the joint update of up to 64 range-bearing observations in one down-date, Jacobians evaluated where the caller says:
// the three slam_ekf_wide_* entry points (include/ext/slamhip_wide.h states the rule; tests/wide_ref.py runs it
// literally).  libslamhip_wide.so.
//
// The front half of the small updates (small_front.h, obs_panel.h) is one workgroup on a 16 x 16 S; this one takes k = 2m <= 128 rows
// as a plain chain of launches on the handle's stream, all arithmetic in double:
//     wide_model_kernel   one thread per observation: the residual at the stored x, the Jacobian blocks Hv | Hf at the linearisation
//                         points (lin / first of a first-estimates object, or the stored x), into the block in Kd
//     wide_s_kernel       one workgroup per observation, one thread per column: S from the stored blocks and 5 x 5 gathers of P,
//                         symmetrised entry by entry, the identity outside the leading k x k; into Smat
//     wide_factor_kernel  ONE workgroup: S in LDS, right-looking Cholesky with small_cholesky's pivot test, inv(L) into the free upper
//                         triangle, y, g, `out`, C (upper, zero padded) and the status word
//     wide_panel_kernel   32 rows a workgroup: the rows of P H' from the gathers of P into LDS, then W1 = (P H') C rounded once and
//                         x += (P H') g; zero rows >= n and zero columns k .. kp; a zero panel when the status word is set
//     launch_downdate     P -= W1 W1' on the plain panel of round_up(k, 16) columns (ekf_syrk.hip), which also keeps Pside
// No workgroup waits for another inside a launch: every dependency is a launch boundary.
//
// The block the observations travel in lies in Kd (free in the Cholesky form; npad kcap >= 4096 doubles).  An observation's Jacobian
// blocks have the layout of obs_panel.h (HB = 10 doubles: Hv 2 x 3 row-major, then Hf 2 x 2), so h_row_dot applies; the state index
// of observation o is 3 + 2 (idf[o] - 1), formed where it is used.
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/ext/slamhip_wide.h"
#include "device_math.h"
#include "fej_object.h"
#include "obs_panel.h"

namespace {

constexpr int WM = SLAM_WIDE_MAXOBS;                       // 64 observations
constexpr int WK = 2 * WM;                                 // 128 rows of S
// the block, in doubles: z[128], R[4] (column-major), idf as int32[64] -- these the host uploads -- then Hv | Hf [64][10] and the
// residual v[128], which the model kernel writes
constexpr int W_Z = 0, W_R = WK, W_IDF = W_R + 4, W_H = W_IDF + WM / 2, W_IN = W_H, W_V = W_H + WM * HB, W_END = W_V + WK;
static_assert(W_END <= SLAM_TILE * SLAM_KPAD, "the block fits the smallest Kd");

// ---- (a) the model -------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(WM) void wide_model_kernel(const T* __restrict__ x, double* __restrict__ blk, int m, const double* __restrict__ lin,
                                                        const double* __restrict__ first) {
    const int o = threadIdx.x;
    if (o >= m) return;
    const int f = 3 + 2 * (reinterpret_cast<const int32_t*>(blk + W_IDF)[o] - 1);
    const ObsModel om = obs_model((double)x[0], (double)x[1], (double)x[2], (double)x[f], (double)x[f + 1]);
    blk[W_V + 2 * o] = blk[W_Z + 2 * o] - om.zp[0];
    blk[W_V + 2 * o + 1] = mpi_to_pi_d(blk[W_Z + 2 * o + 1] - om.zp[1]);
    ObsModel ol = om;                                                     // the Jacobian blocks: at the stored x, or at (lin, first)
    if (lin) ol = obs_model(lin[0], lin[1], lin[2], first[f - 3], first[f - 2]);
    double* hb = blk + W_H + HB * o;
#pragma unroll
    for (int q = 0; q < 6; ++q) hb[q] = ol.Hv[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) hb[6 + q] = ol.Hf[q];
}

// ---- (b) S ---------------------------------------------------------------------------------------------------------------------------
// As s_build_kernel (ekf_update.hip) forms it, but from the stored blocks: workgroup i owns rows 2i, 2i + 1, thread b column b.  The
// entry S[2i + ra][b] and its mirror S[b][2i + ra] are both formed here from the same 25 values of P (the stored matrix is symmetric
// entry for entry), with the expressions the owner of the mirror uses, so that S leaves this kernel symmetric bit for bit.
template <typename T>
__global__ __launch_bounds__(WK) void wide_s_kernel(const T* __restrict__ P, int ld, const double* __restrict__ blk, int m, int kp,
                                                    double* __restrict__ Sg) {
    constexpr int L = kTileLog2<T>;
    __shared__ double hs[WM * HB];
    const int i = blockIdx.x, b = threadIdx.x, k = 2 * m;
    double* row0 = Sg + (size_t)(2 * i) * kp;
    double* row1 = row0 + kp;
    if (i >= m) {                                                         // padding rows: the identity
        if (b < kp) {
            row0[b] = b == 2 * i ? 1.0 : 0.0;
            row1[b] = b == 2 * i + 1 ? 1.0 : 0.0;
        }
        return;
    }
    for (int t = b; t < m * HB; t += WK) hs[t] = blk[W_H + t];
    __syncthreads();
    if (b >= kp) return;
    if (b >= k) {                                                         // padding columns
        row0[b] = 0.0;
        row1[b] = 0.0;
        return;
    }
    const int32_t* __restrict__ idf = reinterpret_cast<const int32_t*>(blk + W_IDF);
    const int j = b >> 1, bb = b & 1;
    const int fi = 3 + 2 * (idf[i] - 1), fj = 3 + 2 * (idf[j] - 1);
    const int rows[5] = {0, 1, 2, fi, fi + 1}, cols[5] = {0, 1, 2, fj, fj + 1};
    double pr[5][5], pc[5][5];                                            // P[a_i, a_j] and its transpose: all 25 gathers before the first use
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            pr[t][u] = (double)sym_at(P, ld, L, rows[t], cols[u]);
            pc[u][t] = pr[t][u];
        }
    const double* hi = hs + HB * i;
    const double* hj = hs + HB * j;
    double ph[5];                                                         // (P H')[rows[t]][b]
#pragma unroll
    for (int t = 0; t < 5; ++t) ph[t] = h_row_dot(hj, 0, bb, pr[t]);
    const double* Rs = blk + W_R;
#pragma unroll
    for (int ra = 0; ra < 2; ++ra) {
        double sv = h_row_dot(hi, 0, ra, ph);                             // S[2i + ra][b]
        if (j == i) sv += Rs[bb * 2 + ra];
        double pt[5];                                                     // (P H')[cols[t]][2i + ra]
#pragma unroll
        for (int t = 0; t < 5; ++t) pt[t] = h_row_dot(hi, 0, ra, pc[t]);
        double st = h_row_dot(hj, 0, bb, pt);                             // S[b][2i + ra]
        if (j == i) st += Rs[ra * 2 + bb];
        (ra ? row1 : row0)[b] = b == 2 * i + ra ? sv : (sv + st) * 0.5;
    }
}

// ---- (c) the factor ------------------------------------------------------------------------------------------------------------------
// ONE workgroup of 1024.  LDS (dynamic): M[kp][kp + 1], then v, y, dinv, e of kp doubles each: kp (kp + 5) doubles, 133 KB at kp = 128.
// The lower triangle of M becomes L, in place; inv(L) goes, transposed, into the strict upper triangle that the factorisation never
// reads (M[c][r] = inv(L)[r][c], r > c) and its diagonal into dinv, so that one matrix holds both.  Every decision is taken from
// values all threads read from LDS after a barrier: uniform.
constexpr int WF_THREADS = 1024;
static inline size_t wide_factor_lds(int kp) { return sizeof(double) * (size_t)kp * (kp + 5); }

__global__ __launch_bounds__(WF_THREADS) void wide_factor_kernel(const double* __restrict__ Sg, const double* __restrict__ blk, int k, int kp,
                                                                 double* __restrict__ Cout, double* __restrict__ gout,
                                                                 double* __restrict__ out4, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldm = kp + 1, tid = threadIdx.x;
    double* M = reinterpret_cast<double*>(smem);
    double* v = M + kp * ldm;
    double* y = v + kp;
    double* dinv = y + kp;
    double* e = dinv + kp;
    for (int t = tid; t < kp * kp; t += WF_THREADS) {
        const int r = t / kp;
        M[r * ldm + (t - r * kp)] = Sg[t];
    }
    if (tid < kp) v[tid] = tid < k ? blk[W_V + tid] : 0.0;
    __syncthreads();
    // right-looking Cholesky, small_cholesky's three barriers a pivot; the trailing update on a 32 x 32 grid of threads
    const int ti = tid >> 5, tj = tid & 31;
    int fail = -1;
    double piv = 0.0, lmin = INFINITY;
    for (int c = 0; c < k; ++c) {
        piv = M[c * ldm + c];
        if (!(piv > 0.0) || !(piv < INFINITY)) { fail = c; break; }
        const double d = sqrt(piv);
        lmin = d < lmin ? d : lmin;
        __syncthreads();
        if (tid >= c && tid < k) M[tid * ldm + c] = M[tid * ldm + c] / d;
        __syncthreads();
        for (int r = c + 1 + ti; r < k; r += 32) {
            const double lrc = M[r * ldm + c];
            for (int q = c + 1 + tj; q <= r; q += 32) M[r * ldm + q] -= lrc * M[q * ldm + c];
        }
        __syncthreads();
    }
    if (fail >= 0) {
        if (tid == 0) {
            out4[0] = 0.0; out4[1] = 0.0; out4[2] = piv; out4[3] = (double)fail;
            if (status) status[0] = 1;
        }
        return;
    }
    if (tid < k) {       // inv(L): thread c solves L X[:, c] = e_c (small_solve's order of terms)
        const int c = tid;
        double dc = 0.0;
        for (int r = c; r < k; ++r) {
            double s = r == c ? 1.0 : 0.0;
            if (r > c) {
                s -= M[r * ldm + c] * dc;
                for (int q = c + 1; q < r; ++q) s -= M[r * ldm + q] * M[c * ldm + q];
            }
            s /= M[r * ldm + r];
            if (r == c) dc = s;
            else M[c * ldm + r] = s;
        }
        dinv[c] = dc;
    }
    __syncthreads();
    if (tid < k) {       // y = inv(L) v
        double s = 0.0;
        for (int q = 0; q < tid; ++q) s += M[q * ldm + tid] * v[q];
        s += dinv[tid] * v[tid];
        y[tid] = s;
        e[tid] = log(M[tid * ldm + tid]);
    }
    __syncthreads();
    if (tid < kp) {      // g = inv(L)' y
        double s = 0.0;
        if (tid < k) {
            s = dinv[tid] * y[tid];
            for (int q = tid + 1; q < k; ++q) s += M[tid * ldm + q] * y[q];
        }
        if (status) gout[tid] = s;
    }
    if (tid == 0) {
        double nis = 0.0, lsum = 0.0;
        for (int q = 0; q < k; ++q) {
            nis += y[q] * y[q];
            lsum += e[q];
        }
        out4[0] = nis; out4[1] = 2.0 * lsum; out4[2] = lmin; out4[3] = -1.0;
        if (status) status[0] = 0;
    }
    if (!status) return;                                                  // nis: the four numbers only
    for (int t = tid; t < kp * kp; t += WF_THREADS) {                     // C[i][j] = inv(L)[j][i], zero outside the leading k x k
        const int i = t / kp, j = t - i * kp;
        Cout[t] = j >= k || j < i ? 0.0 : (i == j ? dinv[i] : M[i * ldm + j]);
    }
}

// ---- (d) the panel -------------------------------------------------------------------------------------------------------------------
// 32 rows of the PANEL a workgroup (npad rows: the rows >= n are written as zero, the down-date has no row guards), 256 threads.
//   phase 1: thread (row, og) gathers P[r, 0:3] and the pairs P[r, f : f + 2] of the observations og, og + 8, ... (all loads issued
//            before the first use; consecutive lanes read consecutive rows of one column wherever (r, f) lies on or below the
//            diagonal tiles -- pht_body's access pattern) and leaves (P H')[r, 0:k] in LDS, column-major.  A landmark named twice is
//            gathered twice, the second time from the cache.
//   phase 2: the columns in groups of 8; thread (row, pg) takes group pg and group ng - 1 - pg -- C is upper triangular, so the pair
//            costs the same for every pg -- and forms W1[r, group] = (P H')[r, :] C[:, group] in double, rounded once.  C is read from
//            global memory: all lanes of a half-wave read the same 64 bytes.  The first 32 threads also form x[r] += (P H')[r, :] g.
// Plain FMAs; the MFMA form (16-row groups per wave, C staged through LDS) is not built.
constexpr int WP_ROWS = 32, WP_THREADS = 256, WP_OG = WP_THREADS / WP_ROWS, WP_PER = WM / WP_OG;      // 8 groups, 8 observations each

template <typename T>
__global__ __launch_bounds__(WP_THREADS) void wide_panel_kernel(T* __restrict__ x, const T* __restrict__ P, int ld, int n,
                                                                const double* __restrict__ blk, int m, int kp, const double* __restrict__ Cin,
                                                                const double* __restrict__ gin, T* __restrict__ W1, int pitchW,
                                                                const int32_t* __restrict__ status) {
    constexpr int L = kTileLog2<T>;
    __shared__ double pht[WK][WP_ROWS];
    __shared__ double hs[WM * HB], gs[WK];
    __shared__ int fs[WM];
    const int tid = threadIdx.x, row = tid & (WP_ROWS - 1), og = tid / WP_ROWS, k = 2 * m;
    const int r = blockIdx.x * WP_ROWS + row;                             // < npad: the grid is npad / 32
    T* __restrict__ w = W1 + (size_t)r * pitchW;
    const bool bad = status[0] != 0;                                      // (uniform)
    if (bad || blockIdx.x * WP_ROWS >= n) {                               // a zero panel; x untouched
        for (int c = og; c < kp; c += WP_OG) w[c] = (T)0;
        return;
    }
    for (int t = tid; t < m * HB; t += WP_THREADS) hs[t] = blk[W_H + t];
    if (tid < WK) gs[tid] = tid < k ? gin[tid] : 0.0;
    if (tid < WM) fs[tid] = 3 + 2 * (reinterpret_cast<const int32_t*>(blk + W_IDF)[tid < m ? tid : 0] - 1);
    __syncthreads();
    const bool live = r < n;
    {
        T t0 = (T)0, t1 = (T)0, t2 = (T)0, q0[WP_PER], q1[WP_PER];
        if (live) {
            t0 = P[p_off(ld, L, r, 0)];
            t1 = P[p_off(ld, L, r, 1)];
            t2 = P[p_off(ld, L, r, 2)];
        }
#pragma unroll
        for (int s = 0; s < WP_PER; ++s) {
            const int o = og + WP_OG * s;
            q0[s] = (T)0;
            q1[s] = (T)0;
            if (live && o < m) {
                q0[s] = sym_at(P, ld, L, r, fs[o]);                       // P[r, f]: from row f where (r, f) lies above the diagonal tiles
                q1[s] = sym_at(P, ld, L, r, fs[o] + 1);
            }
        }
        const double p0 = (double)t0, p1 = (double)t1, p2 = (double)t2;
#pragma unroll
        for (int s = 0; s < WP_PER; ++s) {
            const int o = og + WP_OG * s;
            if (o < m) {
                const double* hb = hs + HB * o;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const double* hv = hb + 3 * q;
                    const double* hf = hb + 6 + 2 * q;
                    pht[2 * o + q][row] = __builtin_fma(hf[1], (double)q1[s], __builtin_fma(hf[0], (double)q0[s],
                                          __builtin_fma(hv[2], p2, __builtin_fma(hv[1], p1, hv[0] * p0))));
                }
            }
        }
    }
    __syncthreads();
    const int k16 = (k + 15) & ~15, ng = k16 / 8;                         // groups of 8 columns, an even number of them
    for (int half = 0; half < 2; ++half) {
        const int grp = half ? ng - 1 - og : og;
        if (og >= ng / 2) break;
        const int c0 = 8 * grp, qend = c0 + 8 < k ? c0 + 8 : k;           // C[q][c] = 0 for q > c
        double acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.0;
        if (live) {
            const double* __restrict__ crow = Cin + c0;
            for (int q = 0; q < qend; ++q) {
                const double a = pht[q][row];
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = __builtin_fma(a, crow[(size_t)q * kp + c], acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c0 + c] = (T)acc[c];
    }
    for (int c = k16 + og; c < kp; c += WP_OG) w[c] = (T)0;               // the columns the panel's pitch pads
    if (og == 0 && live) {
        double dx = 0.0;
        for (int q = 0; q < k; ++q) dx = __builtin_fma(pht[q][row], gs[q], dx);
        x[r] = (T)((double)x[r] + dx);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
template <typename T>
int enqueue(slam_ekf* h, const slam_ekf_fej* f, int m, bool commit) {
    const int k = 2 * m, kp = round_up(k, SLAM_KPAD), k16 = round_up(k, 16);
    double* blk = h->Kd;
    {
        KTimer t(h, SLAM_K_PHT);
        hipLaunchKernelGGL(wide_model_kernel<T>, dim3(1), dim3(WM), 0, h->stream, (const T*)h->x, blk, m, f ? (const double*)f->lin : nullptr,
                           f ? (const double*)f->first : nullptr);
    }
    HIP_TRY(hipGetLastError());
    {
        KTimer t(h, SLAM_K_PHT);
        hipLaunchKernelGGL(wide_s_kernel<T>, dim3(kp / 2), dim3(WK), 0, h->stream, (const T*)h->P, h->ld, (const double*)blk, m, kp, h->Smat);
    }
    HIP_TRY(hipGetLastError());
    {
        KTimer t(h, SLAM_K_FACTOR);
        hipLaunchKernelGGL(wide_factor_kernel, dim3(1), dim3(WF_THREADS), wide_factor_lds(kp), h->stream, (const double*)h->Smat,
                           (const double*)blk, k, kp, h->Cmat, h->gvec, h->d_small, commit ? h->d_status : (int32_t*)nullptr);
    }
    HIP_TRY(hipGetLastError());
    if (!commit) return SLAM_OK;
    {
        KTimer t(h, SLAM_K_W1);
        hipLaunchKernelGGL(wide_panel_kernel<T>, dim3(h->npad / WP_ROWS), dim3(WP_THREADS), 0, h->stream, (T*)h->x, (const T*)h->P, h->ld,
                           3 + 2 * h->N, (const double*)blk, m, kp, (const double*)h->Cmat, (const double*)h->gvec, (T*)h->W1, 2 * h->kcap,
                           (const int32_t*)h->d_status);
    }
    HIP_TRY(hipGetLastError());
    return launch_downdate(h, k16, h->W1, h->W1, 2 * h->kcap, (const int32_t*)nullptr, 0, k16, nullptr);
}

int wide_call(slam_ekf* h, const slam_ekf_fej* f, const double* zf, const int32_t* idf, int m, const double* R, double* out, bool commit) {
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK(zf != nullptr && idf != nullptr && R != nullptr && out != nullptr, "null argument");
    ARG_CHECK(m >= 1 && m <= SLAM_WIDE_MAXOBS, "m outside 1 .. SLAM_WIDE_MAXOBS");
    ARG_CHECK(slam_all_finite(zf, 2 * m), "zf is not finite");
    int rc;
    if ((rc = check_R(R))) return rc;
    if (f) {
        ARG_CHECK(f->h == h, "the first-estimates object belongs to another state");
        ARG_CHECK(f->N == h->N, "the map changed outside the object (its landmark count differs from the state's): call slam_ekf_fej_remap");
    }
    std::vector<double> blob(W_IN, 0.0);
    int32_t* words = reinterpret_cast<int32_t*>(blob.data() + W_IDF);
    for (int o = 0; o < WM; ++o) words[o] = 1;
    for (int o = 0; o < m; ++o) {
        ARG_CHECK(idf[o] >= 1 && idf[o] <= h->N, "idf entry out of range (Julia: BoundsError)");
        words[o] = idf[o];
        blob[W_Z + 2 * o] = zf[2 * o];
        blob[W_Z + 2 * o + 1] = zf[2 * o + 1];
    }
    for (int q = 0; q < 4; ++q) blob[W_R + q] = R[q];
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = ensure_update_workspace(h, m))) return rc;                  // kcap >= round_up(2m, 32): S, C, g and the panel's columns
    // S at kp = 128 needs 133 KB of the CU's 160 KiB of LDS
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&wide_factor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)wide_factor_lds(WK)));
    SlamDrainOnExit drain{h->stream};
    HIP_TRY(hipMemcpyAsync(h->Kd, blob.data(), sizeof(double) * W_IN, hipMemcpyHostToDevice, h->stream));
    rc = h->dtype == SLAM_F32 ? enqueue<float>(h, f, m, commit) : enqueue<double>(h, f, m, commit);
    if (rc) return rc;
    if (commit) h->grid_force = 1;                                        // the means moved: the grid is rebuilt at the next query
    if ((rc = slam_small_out(h, out, 4, 3)) == SLAM_E_NOTPD)
        slam_set_error("wide update: S is not positive definite, pivot %d is %g (state left unchanged)", (int)out[3], out[2]);
    return rc;
}

}  // namespace

extern "C" int slam_ekf_wide_update(slam_ekf_t h, slam_ekf_fej_t f, const double* zf, const int32_t* idf, int m, const double R[4],
                                    double out[4]) {
    SLAM_RANGE();
    return wide_call(h, f, zf, idf, m, R, out, true);
}

extern "C" int slam_ekf_wide_nis(slam_ekf_t h, slam_ekf_fej_t f, const double* zf, const int32_t* idf, int m, const double R[4],
                                 double out[4]) {
    SLAM_RANGE();
    return wide_call(h, f, zf, idf, m, R, out, false);
}

extern "C" int slam_ekf_wide_limits(int32_t out[1]) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr, "null argument");
    out[0] = SLAM_WIDE_MAXOBS;
    return SLAM_OK;
}
