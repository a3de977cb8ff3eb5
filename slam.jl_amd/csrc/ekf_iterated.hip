// ekf_iterated.hip -- the iterated EKF update: slam_ekf_update_iterated, slam_ekf_iterated_nis and slam_ekf_iterated_limits
// (include/ext/slamhip_iterated.h states the rule; tests/iterated_ref.py runs it literally).  libslamhip_iterated.so.
//
// H touches the vehicle and the m <= 8 observed landmarks only, and the iterates of those 3 + 2m states depend on P only through
// the block P[a, a] (at most 19 x 19), so every relinearisation runs inside ONE workgroup and the map is touched once, at the end:
//     iterated_solve_kernel  (one workgroup)       gathers P[a, a] and x0[a] into LDS and runs the whole Gauss-Newton loop there:
//                                                   the model at x_i, v_i, S_i, chol, g_i, x_{i+1}, the step, the cost; leaves
//                                                   C = inv(chol(S)), g, the LAST iteration's Jacobian blocks and `out`
//     iterated_panel_kernel  (a thread per row r)   PHt[r, :] from P[r, 0:3] (read once) and P[r, f : f + 2] of every DISTINCT
//                                                   landmark, W1[r, :] = PHt[r, :] C as the handle's dtype, zero-padded to 16
//                                                   columns, x[r] += PHt[r, :] g
//     launch_downdate                               P -= W1 W1' on the plain 16-column panel (ekf_syrk.hip), which also keeps Pside
// The observations travel in one small block copied into the handle's update workspace (Smat, free in the reference form); the
// solve kernel appends the Jacobian blocks to it, so H never visits the host.  When an S is not positive definite the solve kernel
// sets the handle's status word: the panel kernel then writes a ZERO panel and leaves x alone, and the down-date returns at once on
// the same word.  What is not the loop itself is shared: the block's layout, the gather, P[a, a] H', the entry of S and the panel
// kernel with ekf_fej.hip (obs_panel.h); the factorisation and the solve with that file and ekf_linear.hip (small_front.h).
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/ext/slamhip_iterated.h"
#include "device_math.h"
#include "obs_panel.h"

namespace {

constexpr int OUTN = 10;

// the model at the reduced iterate xs for observation o: its Jacobian blocks and r = z - zp with the bearing wrapped once
__device__ __forceinline__ void eval_model(const double* xs, const double* zs, int o, double* hb, double* r) {
    const ObsModel om = obs_model(xs[0], xs[1], xs[2], xs[3 + 2 * o], xs[4 + 2 * o]);
#pragma unroll
    for (int q = 0; q < 6; ++q) hb[q] = om.Hv[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) hb[6 + q] = om.Hf[q];
    r[0] = zs[2 * o] - om.zp[0];
    r[1] = mpi_to_pi_d(zs[2 * o + 1] - om.zp[1]);
}

// One workgroup of 256, the Gauss-Newton loop around the pieces of obs_panel.h and small_front.h.  Every decision (a failing pivot,
// the stop) is taken from values all threads read from LDS, so it is uniform.  status may be null (the dry run).
template <typename T>
__global__ __launch_bounds__(256) void iterated_solve_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld, double* __restrict__ blob,
                                                              int m, int max_iter, double tol, double* __restrict__ Cout,
                                                              double* __restrict__ gout, double* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ double Pa[NA][NA + 1], PaHt[NA][LP], M[LK][LP], S0[LK][LP], Li[LK][LP];
    __shared__ double x0a[NA], xi[NA], xn[NA], du[NA], v[LK], y[LK], g[LK], pr[LK], rr[2][LK], hb[2][MO][HB], zs[LK], Rs[4];
    __shared__ int cols[NA];
    const int tid = threadIdx.x, k = 2 * m, na = 3 + 2 * m;
    obs_tables(blob, m, cols, zs, Rs);
    obs_gather(x, P, ld, cols, na, Pa, x0a);
    if (tid < na) xi[tid] = x0a[tid];
    __syncthreads();
    if (tid < m) eval_model(xi, zs, tid, hb[0][tid], &rr[0][2 * tid]);
    __syncthreads();
    const double rdet = 1.0 / (Rs[0] * Rs[3] - Rs[1] * Rs[2]);
    const int i = tid >> 4, j = tid & 15;
    int b = 0, it = 0, conv = 0, fail = -1;
    double step = 0.0, nis = 0.0, lsum = 0.0, lmin = 0.0, piv = 0.0, Jfirst = 0.0, Jlast = 0.0;
    for (;;) {
        if (tid < na) du[tid] = x0a[tid] - xi[tid];
        __syncthreads();
        if (tid < k) v[tid] = rr[b][tid] - h_row_dot(hb[b][tid >> 1], tid >> 1, tid & 1, du);      // v = r - H (x0 - x_i)
        obs_paht(hb[b], Pa, PaHt, k, na);
        __syncthreads();
        M[i][j] = obs_s_entry(hb[b], PaHt, Rs, k, i, j);
        S0[i][j] = small_symmetrise(M);                                       // (read after the next barriers)
        // log det S is taken from the factor's diagonal once, after the last iteration
        if ((fail = small_cholesky(M, k, piv, lmin, nullptr)) >= 0) break;
        const double gl = small_solve(M, Li, v, y, k);
        if (tid < LK) g[tid] = gl;
        __syncthreads();
        if (tid < na) {      // x_{i+1} = x0 + P[a, a] H' g
            double s = 0.0;
            for (int q = 0; q < k; ++q) s += PaHt[tid][q] * g[q];
            xn[tid] = x0a[tid] + s;
        }
        if (tid >= 64 && tid < 64 + LK) {      // the prior's share of the cost, row by row: g_t ((S - I (x) R) g)_t
            const int t = tid - 64;
            double s = 0.0;
            if (t < k)
                for (int q = 0; q < k; ++q) s += (S0[t][q] - ((t >> 1) == (q >> 1) ? Rs[(q & 1) * 2 + (t & 1)] : 0.0)) * g[q];
            pr[t] = t < k ? g[t] * s : 0.0;
        }
        __syncthreads();
        if (tid < m) eval_model(xn, zs, tid, hb[b ^ 1][tid], &rr[b ^ 1][2 * tid]);      // the cost's residuals; the next iteration's model
        step = 0.0;
        for (int r = 0; r < na; ++r) {
            const double d = fabs(xn[r] - xi[r]);
            step = d > step ? d : step;
        }
        nis = 0.0;
        for (int q = 0; q < k; ++q) nis += y[q] * y[q];
        __syncthreads();
        double J = 0.0;
        for (int q = 0; q < k; ++q) J += pr[q];
        for (int o = 0; o < m; ++o) {
            const double r0 = rr[b ^ 1][2 * o], r1 = rr[b ^ 1][2 * o + 1];
            J += (Rs[3] * r0 * r0 - (Rs[1] + Rs[2]) * r0 * r1 + Rs[0] * r1 * r1) * rdet;
        }
        if (it == 0) Jfirst = J;
        Jlast = J;
        ++it;
        conv = step <= tol;
        if (conv || it == max_iter) break;
        if (tid < na) xi[tid] = xn[tid];
        b ^= 1;
        __syncthreads();
    }
    if (fail >= 0) {
        if (tid == 0) {
            out[0] = (double)it; out[1] = 0.0; out[2] = step; out[3] = 0.0; out[4] = 0.0; out[5] = piv; out[6] = (double)fail;
            out[7] = (double)it; out[8] = Jfirst; out[9] = Jlast;
            if (status) status[0] = 1;
        }
        return;
    }
    small_store_c(Li, k, Cout);
    if (tid < LK) gout[tid] = tid < k ? g[tid] : 0.0;
    if (tid < m * HB) blob[B_H + tid] = hb[b][tid / HB][tid % HB];       // the Jacobian of the LAST iteration, for the panel
    if (tid == 0) {
        for (int c = 0; c < k; ++c) lsum += log(M[c][c]);                 // the last iteration's factor is still in M
        out[0] = (double)it; out[1] = conv ? 1.0 : 0.0; out[2] = step; out[3] = nis; out[4] = 2.0 * lsum; out[5] = lmin; out[6] = -1.0;
        out[7] = -1.0; out[8] = Jfirst; out[9] = Jlast;
        if (status) status[0] = 0;
    }
}


// every rule of the header; fills the block.  h is dereferenced only after the rules that need no state
int check_arguments(slam_ekf* h, const double* zf, const int32_t* idf, int m, const double* R, int max_iter, double tol, const double* out,
                    std::vector<double>& blob) {
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK(zf != nullptr && idf != nullptr && R != nullptr && out != nullptr, "null argument");
    ARG_CHECK(m >= 1 && m <= SLAM_ITERATED_MAXOBS, "m outside 1 .. SLAM_ITERATED_MAXOBS");
    ARG_CHECK(max_iter >= 1 && max_iter <= SLAM_ITERATED_MAXITER, "max_iter outside 1 .. 64");
    ARG_CHECK(std::isfinite(tol) && tol >= 0.0, "tol is negative or not finite");
    ARG_CHECK(slam_all_finite(zf, 2 * m), "zf is not finite");
    int rc;
    if ((rc = check_R(R))) return rc;
    return obs_block_fill(h, zf, idf, m, R, blob);
}

template <typename T>
int enqueue(slam_ekf* h, int m, int max_iter, double tol, bool commit) {
    {
        KTimer t(h, SLAM_K_FACTOR);
        hipLaunchKernelGGL(iterated_solve_kernel<T>, dim3(1), dim3(256), 0, h->stream, (const T*)h->x, (const T*)h->P, h->ld, h->Smat, m, max_iter,
                           tol, h->Cmat, h->gvec, h->d_small, commit ? h->d_status : (int32_t*)nullptr);
    }
    HIP_TRY(hipGetLastError());
    return commit ? enqueue_obs_panel<T>(h, m) : SLAM_OK;
}

int iterated_call(slam_ekf* h, const double* zf, const int32_t* idf, int m, const double* R, int max_iter, double tol, double* out,
                  bool commit) {
    std::vector<double> blob;
    int rc;
    if ((rc = check_arguments(h, zf, idf, m, R, max_iter, tol, out, blob))) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = ensure_update_workspace(h, MO))) return rc;                 // kcap >= 32: Smat holds the block, W1 16 columns
    SlamDrainOnExit drain{h->stream};
    HIP_TRY(hipMemcpyAsync(h->Smat, blob.data(), sizeof(double) * B_IN, hipMemcpyHostToDevice, h->stream));
    rc = h->dtype == SLAM_F32 ? enqueue<float>(h, m, max_iter, tol, commit) : enqueue<double>(h, m, max_iter, tol, commit);
    if (rc) return rc;
    if (commit) h->grid_force = 1;                                        // the means moved: the grid is rebuilt at the next query
    if ((rc = slam_small_out(h, out, OUTN, 6)) == SLAM_E_NOTPD)
        slam_set_error("iterated update: S is not positive definite at iteration %d, pivot %d is %g (state left unchanged)", (int)out[7],
                       (int)out[6], out[5]);
    return rc;
}

}  // namespace

extern "C" int slam_ekf_update_iterated(slam_ekf_t h, const double* zf, const int32_t* idf, int m, const double R[4], int max_iter,
                                        double tol, double out[10]) {
    SLAM_RANGE();
    return iterated_call(h, zf, idf, m, R, max_iter, tol, out, true);
}

extern "C" int slam_ekf_iterated_nis(slam_ekf_t h, const double* zf, const int32_t* idf, int m, const double R[4], int max_iter, double tol,
                                     double out[10]) {
    SLAM_RANGE();
    return iterated_call(h, zf, idf, m, R, max_iter, tol, out, false);
}

extern "C" int slam_ekf_iterated_limits(int32_t out[2]) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr, "null argument");
    out[0] = SLAM_ITERATED_MAXOBS;
    out[1] = SLAM_ITERATED_MAXITER;
    return SLAM_OK;
}
