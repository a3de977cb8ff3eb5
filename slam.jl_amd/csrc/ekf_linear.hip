// ekf_linear.hip -- caller-supplied models for the EKF: slam_ekf_update_linear, slam_ekf_linear_nis, slam_ekf_predict_linear and
// slam_ekf_predict_odometry (include/ext/slamhip_linear.h states the rules; tests/linear_ref.py runs them literally).
// libslamhip_linear.so.
//
// UPDATE.  The reference's Cholesky-form update (src/ekf.jl:67-75) for k <= 16 sparse rows of H in CSR, the shape of the merge
// (ekf_merge.hip) with the caller's rows in place of +I2 / -I2:
//     linear_factor_kernel  (one workgroup)       S = H P H' + R entry by entry from the symmetric view of P, then the pieces of
//                                                  small_front.h: symmetrised, chol, C = inv(chol(S)), g = C C' v; the four
//                                                  numbers of `out`; all in double
//     linear_panel_kernel   (a thread per row r)   PHt[r, :] from the row's <= 8 non-zeros, W1[r, :] = PHt[r, :] C as the handle's
//                                                  dtype, zero-padded to 16 columns, x[r] += PHt[r, :] g
//     launch_downdate                              P -= W1 W1' on the plain 16-column panel (ekf_syrk.hip), which also keeps Pside
// The measurement travels in one block of 474 doubles (LinBlob) copied into the handle's update workspace (Smat, free in the
// reference form), so that the kernels index it freely.  When S is not positive definite the factor kernel sets the handle's
// status word: the panel kernel then writes a ZERO panel and leaves x alone, and the down-date returns at once on the same word.
//
// PREDICT.  linear_strip_kernel, one launch over the vehicle's three columns of the tile-major matrix as predict_kernel
// (ekf_strip.hip) walks them: thread f >= 3 owns row f of the column strip and its mirror; the workgroup that arrives last, i.e.
// after every workgroup has read the heading, rewrites P_vv and the pose (strip_tail.h).  Gv and Qv come from the caller (predict_linear) or
// are formed from x[2] and the increment on the device (predict_odometry).
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/ext/slamhip_linear.h"
#include "device_math.h"
#include "small_front.h"
#include "strip_tail.h"

namespace {

static_assert(SLAM_LINEAR_MAXROWS == LK, "the rows fill the 16 x 16 front half");
constexpr int LNZ = SLAM_LINEAR_MAXROWS * SLAM_LINEAR_MAXNNZ;
// LinBlob, in doubles: R as 16 x 16 (symmetric, zero outside k x k), z, val, then int32 words: ptr[17] and, from word 20, idx[128]
constexpr int B_R = 0, B_Z = LK * LK, B_VAL = B_Z + LK, B_INT = B_VAL + LNZ, B_IDX_WORD = 20;
constexpr int B_DOUBLES = B_INT + (B_IDX_WORD + LNZ) / 2;

// the rows' tables from the blob into LDS; rows >= k are empty
__device__ __forceinline__ void linear_tables(const double* __restrict__ blob, int k, int* sptr, int* sidx, double* sval) {
    const int32_t* __restrict__ words = reinterpret_cast<const int32_t*>(blob + B_INT);
    for (int t = threadIdx.x; t <= LK; t += blockDim.x) sptr[t] = words[t < k ? t : k];
    for (int t = threadIdx.x; t < LNZ; t += blockDim.x) {
        sidx[t] = words[B_IDX_WORD + t];
        sval[t] = blob[B_VAL + t];
    }
    __syncthreads();
}

// (P H')[r, row]: the row's non-zeros b0 .. b0 + cnt - 1, cnt >= 1, in the order given.  Always SLAM_LINEAR_MAXNNZ loads, the ones
// past the row's end at the address of its first (a hit in the cache) with weight zero: a fixed trip count, so that the loads --
// dependent-latency gathers, half of them strided -- are in flight together instead of one behind the other.
template <typename T>
__device__ __forceinline__ double linear_pht(const T* __restrict__ P, int ld, int L, int r, int b0, int cnt, const int* sidx,
                                             const double* sval) {
    double pv[SLAM_LINEAR_MAXNNZ];
#pragma unroll
    for (int a = 0; a < SLAM_LINEAR_MAXNNZ; ++a) pv[a] = (double)sym_at(P, ld, L, r, sidx[a < cnt ? b0 + a : b0]);
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < SLAM_LINEAR_MAXNNZ; ++a)
        if (a < cnt) s += pv[a] * sval[b0 + a];
    return s;
}

// One workgroup of 256: thread (i, j) forms S[i][j], lane i of the first 16 v[i]; small_front.h does the rest.  out4 = {v' inv(S) v,
// log det S, min l_jj, -1} or, when pivot j fails, {0, 0, d_j, j} and nothing else is written.  log det S is summed, ascending, over
// the l_jj as the chain took their square roots: they wait in y, which is free until the solve, and a lane of the second wave --
// idle while the first inverts L -- takes the logarithms.  status (may be null: the gate alone) gets 0 / 1.
template <typename T>
__global__ __launch_bounds__(256) void linear_factor_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld,
                                                             const double* __restrict__ blob, int k, int mode, unsigned wrap,
                                                             double* __restrict__ Cout, double* __restrict__ gout,
                                                             double* __restrict__ out4, int32_t* __restrict__ status) {
    constexpr int L = kTileLog2<T>;
    __shared__ double M[LK][LP], Li[LK][LP], v[LK], y[LK], sval[LNZ];
    __shared__ int sptr[LK + 1], sidx[LNZ];
    const int tid = threadIdx.x;
    linear_tables(blob, k, sptr, sidx, sval);
    const int i = tid >> 4, j = tid & 15;
    {
        double s = i == j ? 1.0 : 0.0;
        if (i < k && j < k) {
            double acc = 0.0;                                             // H[i, :] (P H')[:, j]
            const int b0 = sptr[j], cnt = sptr[j + 1] - b0;
            for (int a = sptr[i]; a < sptr[i + 1]; ++a) acc += sval[a] * linear_pht(P, ld, L, sidx[a], b0, cnt, sidx, sval);
            s = acc + blob[B_R + i * LK + j];
        }
        M[i][j] = s;
    }
    if (tid < LK) {
        double d = 0.0;
        if (tid < k) {
            d = blob[B_Z + tid];
            if (mode == SLAM_LINEAR_MEASURED) {
                double hx = 0.0;
                for (int a = sptr[tid]; a < sptr[tid + 1]; ++a) hx += sval[a] * (double)x[sidx[a]];
                d -= hx;
                if ((wrap >> tid) & 1u) d = mpi_to_pi_d(d);
            }
        }
        v[tid] = d;
    }
    small_symmetrise(M);
    double piv = 0.0, lmin;
    const int fail = small_cholesky(M, k, piv, lmin, y);
    if (fail >= 0) {
        if (tid == 0) {
            out4[0] = 0.0; out4[1] = 0.0; out4[2] = piv; out4[3] = (double)fail;
            if (status) status[0] = 1;
        }
        return;
    }
    if (tid == 64) {
        double lsum = 0.0;
        for (int c = 0; c < k; ++c) lsum += log(y[c]);
        out4[1] = 2.0 * lsum;
    }
    const double gl = small_solve(M, Li, v, y, k);
    if (tid < LK) gout[tid] = gl;
    small_store_c(Li, k, Cout);
    if (tid == 0) {
        double nis = 0.0;
        for (int m = 0; m < k; ++m) nis += y[m] * y[m];
        out4[0] = nis; out4[2] = lmin; out4[3] = -1.0;
        if (status) status[0] = 0;
    }
}

// One thread per row r of the PANEL (npad rows: the rows >= n are written as zero, the down-date has no row guards).  A row costs
// up to 128 dependent-latency loads, half of them strided (the transposed side of the symmetric view), so the rows are spread over
// as many CUs as there are: one wave a workgroup.
constexpr int PANEL_THREADS = 64;

template <typename T>
__global__ __launch_bounds__(PANEL_THREADS) void linear_panel_kernel(T* __restrict__ x, const T* __restrict__ P, int ld, int n, int npad,
                                                            const double* __restrict__ blob, int k, const double* __restrict__ Cin,
                                                            const double* __restrict__ gin, T* __restrict__ W1, int pitchW,
                                                            const int32_t* __restrict__ status) {
    constexpr int L = kTileLog2<T>;
    __shared__ double Cs[LK * LK], gs[LK], sval[LNZ];
    __shared__ int sptr[LK + 1], sidx[LNZ];
    const bool bad = status[0] != 0;                                      // (uniform)
    linear_tables(blob, k, sptr, sidx, sval);
    if (!bad) {
        for (int t = threadIdx.x; t < LK * LK; t += PANEL_THREADS) Cs[t] = Cin[t];
        if (threadIdx.x < LK) gs[threadIdx.x] = gin[threadIdx.x];
    }
    __syncthreads();
    const int r = blockIdx.x * PANEL_THREADS + threadIdx.x;
    if (r >= npad) return;
    T* __restrict__ w = W1 + (size_t)r * pitchW;
    if (bad || r >= n) {
#pragma unroll
        for (int j = 0; j < LK; ++j) w[j] = (T)0;
        return;
    }
    double dxr = 0.0, acc[LK];
#pragma unroll
    for (int j = 0; j < LK; ++j) acc[j] = 0.0;
    for (int i = 0; i < k; ++i) {             // W1[r, j] = sum_{i <= j} PHt[r, i] C[i][j], i ascending (C is upper: zero below)
        const int b0 = sptr[i];
        const double pht = linear_pht(P, ld, L, r, b0, sptr[i + 1] - b0, sidx, sval);
#pragma unroll
        for (int j = 0; j < LK; ++j) acc[j] += pht * Cs[i * LK + j];
        dxr += pht * gs[i];
    }
#pragma unroll
    for (int j = 0; j < LK; ++j) w[j] = (T)acc[j];
    x[r] = (T)((double)x[r] + dxr);
}

struct StripArgs {
    double xv[3];      // the new pose, or the increment d (odo)
    double G[9];       // Gv, column-major (not read: odo)
    double Q[9];       // Qv, or Q3 (odo); column-major, the lower triangle is read
    int odo;
};

template <typename T>
__global__ __launch_bounds__(256) void linear_strip_kernel(T* __restrict__ x, T* __restrict__ P, int ld, int n, StripArgs A,
                                                            int32_t* __restrict__ arrive, int tlog) {
    double G[3][3], xn[3];
    double sn = 0.0, cs = 1.0;
    if (A.odo) {
        const double phi = (double)x[2];
        sn = sin(phi);
        cs = cos(phi);
        const double dx = A.xv[0], dy = A.xv[1];
        const double gx = cs * dx - sn * dy, gy = sn * dx + cs * dy;      // the increment in the map frame
        G[0][0] = 1.0; G[0][1] = 0.0; G[0][2] = -gy;
        G[1][0] = 0.0; G[1][1] = 1.0; G[1][2] = gx;
        G[2][0] = 0.0; G[2][1] = 0.0; G[2][2] = 1.0;
        xn[0] = (double)x[0] + gx;
        xn[1] = (double)x[1] + gy;
        xn[2] = mpi_to_pi_d(phi + A.xv[2]);
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) G[r][c] = A.G[c * 3 + r];
            xn[r] = A.xv[r];
        }
    }
    const int f = 3 + blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n) {
        const double p0 = (double)P[p_off(ld, tlog, f, 0)];
        const double p1 = (double)P[p_off(ld, tlog, f, 1)];
        const double p2 = (double)P[p_off(ld, tlog, f, 2)];
#pragma unroll
        for (int c = 0; c < 3; ++c)       // column strip P[f, 0:3] = P[f, 0:3] Gv'; its mirror exists inside the first tile only
            p_store_sym(P, ld, tlog, f, c, (T)(G[c][0] * p0 + G[c][1] * p1 + G[c][2] * p2));
    }
    if (!strip_arrive_last(arrive) || threadIdx.x != 0) return;
    strip_rearm(arrive);
    double Qs[3][3], Qv[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) Qs[r][c] = Qs[c][r] = A.Q[c * 3 + r];
    if (A.odo) {                              // Qv = Gu Q3 Gu', Gu = blockdiag([cs -sn; sn cs], 1)
        const double Gu[3][3] = {{cs, -sn, 0.0}, {sn, cs, 0.0}, {0.0, 0.0, 1.0}};
        double GQ[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) GQ[r][c] = Gu[r][0] * Qs[0][c] + Gu[r][1] * Qs[1][c] + Gu[r][2] * Qs[2][c];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c <= r; ++c) Qv[r][c] = GQ[r][0] * Gu[c][0] + GQ[r][1] * Gu[c][1] + GQ[r][2] * Gu[c][2];
    } else {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c <= r; ++c) Qv[r][c] = Qs[r][c];
    }
    strip_rewrite_pvv(P, ld, tlog, G, Qv);
    x[0] = (T)xn[0];
    x[1] = (T)xn[1];
    x[2] = (T)xn[2];
}

// every rule of the header that the host can decide; fills the blob.  h is dereferenced only after the rules that need no state
int check_measurement(slam_ekf* h, int k, const int32_t* ptr, const int32_t* idx, const double* val, const double* z, const double* R,
                      int mode, uint32_t wrap_mask, const double* out, std::vector<double>& blob) {
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK(ptr != nullptr && idx != nullptr && val != nullptr && z != nullptr && R != nullptr && out != nullptr, "null argument");
    ARG_CHECK(k >= 1 && k <= SLAM_LINEAR_MAXROWS, "k outside 1 .. SLAM_LINEAR_MAXROWS");
    ARG_CHECK(mode == SLAM_LINEAR_MEASURED || mode == SLAM_LINEAR_INNOVATION, "unknown mode");
    ARG_CHECK(mode == SLAM_LINEAR_MEASURED || wrap_mask == 0, "wrap_mask must be 0 when z is the innovation");
    ARG_CHECK((wrap_mask >> k) == 0, "wrap_mask has bits beyond row k");
    ARG_CHECK(ptr[0] == 0, "ptr[0] must be 0");
    const int n = 3 + 2 * h->N;
    blob.assign(B_DOUBLES, 0.0);
    int32_t* words = reinterpret_cast<int32_t*>(blob.data() + B_INT);
    for (int i = 0; i < k; ++i) {
        const int cnt = ptr[i + 1] - ptr[i];
        ARG_CHECK(cnt >= 1 && cnt <= SLAM_LINEAR_MAXNNZ, "a row has no non-zero or more than SLAM_LINEAR_MAXNNZ");
        for (int a = ptr[i]; a < ptr[i + 1]; ++a) {
            ARG_CHECK(idx[a] >= 0 && idx[a] < n, "state index out of range");
            for (int b = ptr[i]; b < a; ++b) ARG_CHECK(idx[b] != idx[a], "a state index appears twice in one row");
            ARG_CHECK(std::isfinite(val[a]), "val is not finite");
            words[B_IDX_WORD + a] = idx[a];
            blob[B_VAL + a] = val[a];
        }
        words[i + 1] = ptr[i + 1];
    }
    ARG_CHECK(slam_all_finite(z, k), "z is not finite");
    ARG_CHECK(slam_all_finite(R, k * k), "R is not finite");
    for (int i = 0; i < k; ++i) {
        ARG_CHECK(R[i * k + i] >= 0.0, "R has a negative diagonal");
        for (int j = 0; j < k; ++j) {
            ARG_CHECK(R[j * k + i] == R[i * k + j], "R is not symmetric");
            blob[B_R + i * LK + j] = R[j * k + i];
        }
        blob[B_Z + i] = z[i];
    }
    return SLAM_OK;
}

template <typename T>
int enqueue_front(slam_ekf* h, int k, int mode, uint32_t wrap, bool commit) {
    const int n = 3 + 2 * h->N;
    const double* blob = h->Smat;
    {
        KTimer t(h, SLAM_K_FACTOR);
        hipLaunchKernelGGL(linear_factor_kernel<T>, dim3(1), dim3(256), 0, h->stream, (const T*)h->x, (const T*)h->P, h->ld, blob, k, mode,
                           (unsigned)wrap, h->Cmat, h->gvec, h->d_small, commit ? h->d_status : (int32_t*)nullptr);
    }
    HIP_TRY(hipGetLastError());
    if (!commit) return SLAM_OK;
    {
        KTimer t(h, SLAM_K_W1);
        hipLaunchKernelGGL(linear_panel_kernel<T>, dim3((h->npad + PANEL_THREADS - 1) / PANEL_THREADS), dim3(PANEL_THREADS), 0, h->stream, (T*)h->x, (const T*)h->P, h->ld, n,
                           h->npad, blob, k, (const double*)h->Cmat, (const double*)h->gvec, (T*)h->W1, 2 * h->kcap,
                           (const int32_t*)h->d_status);
    }
    HIP_TRY(hipGetLastError());
    return launch_downdate(h, LK, h->W1, h->W1, 2 * h->kcap, (const int32_t*)nullptr, 0, LK, nullptr);
}

int linear_call(slam_ekf* h, int k, const int32_t* ptr, const int32_t* idx, const double* val, const double* z, const double* R, int mode,
                uint32_t wrap_mask, double* out, bool commit) {
    std::vector<double> blob;
    int rc;
    if ((rc = check_measurement(h, k, ptr, idx, val, z, R, mode, wrap_mask, out, blob))) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = ensure_update_workspace(h, SLAM_LINEAR_MAXROWS / 2))) return rc;      // kcap >= 32: Smat holds the blob, W1 16 columns
    SlamDrainOnExit drain{h->stream};
    HIP_TRY(hipMemcpyAsync(h->Smat, blob.data(), sizeof(double) * B_DOUBLES, hipMemcpyHostToDevice, h->stream));
    rc = h->dtype == SLAM_F32 ? enqueue_front<float>(h, k, mode, wrap_mask, commit) : enqueue_front<double>(h, k, mode, wrap_mask, commit);
    if (rc) return rc;
    if (commit) h->grid_force = 1;                                        // the means moved: the grid is rebuilt at the next query
    if ((rc = slam_small_out(h, out, 4, 3)) == SLAM_E_NOTPD)
        slam_set_error("linear measurement: S is not positive definite, pivot %d is %g (state left unchanged)", (int)out[3], out[2]);
    return rc;
}

int strip_call(slam_ekf* h, const StripArgs& A) {
    HIP_TRY(hipSetDevice(h->device));
    const int n = 3 + 2 * h->N;
    const int blocks = h->N > 0 ? (2 * h->N + 255) / 256 : 1;
    int32_t* arrive = h->d_count + 3;                                     // predict_kernel's counter: one stream, left at zero
    {
        KTimer t(h, SLAM_K_PREDICT);
        if (h->dtype == SLAM_F32)
            hipLaunchKernelGGL(linear_strip_kernel<float>, dim3(blocks), dim3(256), 0, h->stream, (float*)h->x, (float*)h->P, h->ld, n, A,
                               arrive, 7);
        else
            hipLaunchKernelGGL(linear_strip_kernel<double>, dim3(blocks), dim3(256), 0, h->stream, (double*)h->x, (double*)h->P, h->ld, n, A,
                               arrive, 6);
    }
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_ekf_update_linear(slam_ekf_t h, int k, const int32_t* ptr, const int32_t* idx, const double* val, const double* z,
                                      const double* R, int mode, uint32_t wrap_mask, double* out) {
    SLAM_RANGE();
    return linear_call(h, k, ptr, idx, val, z, R, mode, wrap_mask, out, true);
}

extern "C" int slam_ekf_linear_nis(slam_ekf_t h, int k, const int32_t* ptr, const int32_t* idx, const double* val, const double* z,
                                   const double* R, int mode, uint32_t wrap_mask, double* out) {
    SLAM_RANGE();
    return linear_call(h, k, ptr, idx, val, z, R, mode, wrap_mask, out, false);
}

extern "C" int slam_ekf_predict_linear(slam_ekf_t h, const double* xv, const double* Gv, const double* Qv) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr && xv != nullptr && Gv != nullptr && Qv != nullptr, "null argument");
    ARG_CHECK(slam_all_finite(xv, 3) && slam_all_finite(Gv, 9) && slam_all_finite(Qv, 9), "a value is not finite");
    StripArgs A;
    memcpy(A.xv, xv, sizeof(A.xv));
    memcpy(A.G, Gv, sizeof(A.G));
    memcpy(A.Q, Qv, sizeof(A.Q));
    A.odo = 0;
    return strip_call(h, A);
}

extern "C" int slam_ekf_predict_odometry(slam_ekf_t h, const double* d, const double* Q3) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr && d != nullptr && Q3 != nullptr, "null argument");
    ARG_CHECK(slam_all_finite(d, 3) && slam_all_finite(Q3, 9), "a value is not finite");
    StripArgs A;
    memset(&A, 0, sizeof(A));
    memcpy(A.xv, d, sizeof(A.xv));
    memcpy(A.Q, Q3, sizeof(A.Q));
    A.odo = 1;
    return strip_call(h, A);
}
