// ekf_fej.hip -- first-estimates Jacobian (FEJ) predict, update and augment: the eleven slam_ekf_fej_* entry points
// (include/ext/slamhip_fej.h states the rule; tests/fej_ref.py runs it literally).  libslamhip_fej.so.
//
// No formula of the filter changes, only where its Jacobians are evaluated: every landmark at its first estimate, the vehicle at
// its predicted pose.  Both live on the device beside the state, as doubles (lin[3], first[2 maxN]), so that no call reads a mean
// back to the host:
//     fej_strip_kernel    predict: one launch over the vehicle's three columns of the tile-major matrix, as predict_kernel
//                         (ekf_strip.hip) walks them.  Every workgroup forms x+ and Gv for itself from the stored pose and lin; the
//                         workgroup that arrives last -- after every workgroup has read both -- rewrites P_vv, the pose and lin
//                         (strip_tail.h)
//     fej_front_kernel    update, one workgroup: gathers P[a, a] (at most 19 x 19), x[a], lin and first[a] into LDS, takes the
//                         residuals at x and the Jacobian blocks at (lin, first), forms S (obs_panel.h), its factor,
//                         C = inv(chol(S)), g and `out` (small_front.h), and leaves the Jacobian blocks in the observation block
//     iterated_panel_kernel (obs_panel.h)   PHt rows, W1 and x += PHt g from those blocks; a zero panel when the status word is set
//     launch_downdate     P -= W1 W1' on the plain 16-column panel (ekf_syrk.hip), which also keeps Pside
//     fej_augment_kernel  augment: augment_kernel (ekf_strip.hip) with Gv = [I | J (lm - lin_xy)], and first <- lm
//     fej_take / fej_remap / fej_transform kernels   the linearisation points taken from x, renumbered, moved into another frame
// No workgroup waits for another inside a launch: every dependency is a launch boundary or the last-arriver counter.
#include <cmath>
#include <new>
#include <vector>

#include "common.h"
#include "../../include/ext/slamhip_fej.h"
#include "device_math.h"
#include "fej_object.h"
#include "obs_panel.h"
#include "strip_tail.h"

namespace {

static_assert(SLAM_FEJ_MAXOBS == MO, "the panel kernel takes 8 observations");

// ---- predict -----------------------------------------------------------------------------------------------------------------------
// As predict_kernel: thread f >= 3 owns row f of the column strip and its mirror.  x+ is rounded to T BEFORE Gv is formed from it,
// so that Gv carries the old linearisation pose exactly onto the new one (lin <- x+ as stored).  The pose and lin are read by every
// workgroup and rewritten by the one that arrives last at the counter (strip_tail.h).
template <typename T>
__global__ __launch_bounds__(256) void fej_strip_kernel(T* __restrict__ x, T* __restrict__ P, int ld, int n, double* __restrict__ lin,
                                                         double v, double g, double w, double Q0, double Q1, double Q2, double Q3,
                                                         double dt, int32_t* __restrict__ arrive, int tlog) {
    const double x0 = (double)x[0], x1 = (double)x[1], phi = (double)x[2];
    const double l0 = lin[0], l1 = lin[1];
    const double sn = sin(g + phi), cs = cos(g + phi);
    const double vts = v * dt * sn, vtc = v * dt * cs;
    const T xp0 = (T)(x0 + vtc), xp1 = (T)(x1 + vts), xp2 = (T)mpi_to_pi_d(phi + v * dt * sin(g) / w);
    const double ga = -((double)xp1 - l1), gb = (double)xp0 - l0;        // J (x+[0:2] - lin[0:2])
    const int f = 3 + blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n) {
        const double p0 = (double)P[p_off(ld, tlog, f, 0)];
        const double p1 = (double)P[p_off(ld, tlog, f, 1)];
        const double p2 = (double)P[p_off(ld, tlog, f, 2)];
        p_store_sym(P, ld, tlog, f, 0, (T)(p0 + ga * p2));                // Gv = [1 0 ga; 0 1 gb; 0 0 1]
        p_store_sym(P, ld, tlog, f, 1, (T)(p1 + gb * p2));
        p_store_sym(P, ld, tlog, f, 2, (T)p2);
    }
    if (!strip_arrive_last(arrive) || threadIdx.x != 0) return;
    strip_rearm(arrive);
    const double Gv[3][3] = {{1.0, 0.0, ga}, {0.0, 1.0, gb}, {0.0, 0.0, 1.0}};
    const double Gu[3][2] = {{dt * cs, -vts}, {dt * sn, vtc}, {dt * sin(g) / w, v * dt * cos(g) / w}};
    double GQG[3][3];
    strip_gu_q_gut(Gu, Q0, Q1, Q2, Q3, GQG);
    strip_rewrite_pvv(P, ld, tlog, Gv, GQG);
    x[0] = xp0;
    x[1] = xp1;
    x[2] = xp2;
    lin[0] = (double)xp0;
    lin[1] = (double)xp1;
    lin[2] = (double)xp2;
}

// ---- update: the front half ----------------------------------------------------------------------------------------------------------
// One workgroup of 256: the two model evaluations between the pieces of obs_panel.h and small_front.h.
template <typename T>
__global__ __launch_bounds__(256) void fej_front_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld, double* __restrict__ blob,
                                                         int m, const double* __restrict__ lin, const double* __restrict__ first,
                                                         double* __restrict__ Cout, double* __restrict__ gout, double* __restrict__ out4,
                                                         int32_t* __restrict__ status) {
    __shared__ double Pa[NA][NA + 1], PaHt[NA][LP], M[LK][LP], Li[LK][LP];
    __shared__ double xa[NA], la[NA], v[LK], y[LK], hb[MO][HB], zs[LK], Rs[4];
    __shared__ int cols[NA];
    const int tid = threadIdx.x, k = 2 * m, na = 3 + 2 * m;
    obs_tables(blob, m, cols, zs, Rs);
    obs_gather(x, P, ld, cols, na, Pa, xa);
    if (tid < na) la[tid] = tid < 3 ? lin[tid] : first[cols[tid] - 3];
    __syncthreads();
    if (tid < m) {            // the residual at the stored mean, the Jacobian blocks at the linearisation points
        const ObsModel om = obs_model(xa[0], xa[1], xa[2], xa[3 + 2 * tid], xa[4 + 2 * tid]);
        v[2 * tid] = zs[2 * tid] - om.zp[0];
        v[2 * tid + 1] = mpi_to_pi_d(zs[2 * tid + 1] - om.zp[1]);
        const ObsModel ol = obs_model(la[0], la[1], la[2], la[3 + 2 * tid], la[4 + 2 * tid]);
#pragma unroll
        for (int q = 0; q < 6; ++q) hb[tid][q] = ol.Hv[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) hb[tid][6 + q] = ol.Hf[q];
    }
    __syncthreads();
    obs_paht(hb, Pa, PaHt, k, na);
    __syncthreads();
    M[tid >> 4][tid & 15] = obs_s_entry(hb, PaHt, Rs, k, tid >> 4, tid & 15);
    small_symmetrise(M);
    double piv = 0.0, lmin;
    const int fail = small_cholesky(M, k, piv, lmin, nullptr);
    if (fail >= 0) {
        if (tid == 0) {
            out4[0] = 0.0; out4[1] = 0.0; out4[2] = piv; out4[3] = (double)fail;
            status[0] = 1;
        }
        return;
    }
    const double gl = small_solve(M, Li, v, y, k);
    if (tid < LK) gout[tid] = gl;
    small_store_c(Li, k, Cout);
    if (tid < m * HB) blob[B_H + tid] = hb[tid / HB][tid % HB];          // the Jacobian blocks, for the panel
    if (tid == 0) {
        double nis = 0.0, lsum = 0.0;
        for (int q = 0; q < k; ++q) {
            nis += y[q] * y[q];
            lsum += log(M[q][q]);
        }
        out4[0] = nis; out4[1] = 2.0 * lsum; out4[2] = lmin; out4[3] = -1.0;
        status[0] = 0;
    }
}

// ---- augment -------------------------------------------------------------------------------------------------------------------------
// augment_kernel (ekf_strip.hip) with the third column of Gv taken from the new mean AS STORED and lin: thread t owns old state index
// c = t and writes, for every new feature a, the cross block P[fa : fa + 2, c] = Gv_a P[0:3, c] and its mirror; block 0 writes the
// new-new blocks, the new entries of x and the new first estimates.
template <typename T>
__device__ __forceinline__ void fej_new_feature(double xv, double yv, double phi, double l0, double l1, const double* __restrict__ zn, int a,
                                                double G[2][3], double Gz[2][2], T* lm) {
    const double r = zn[2 * a], b = zn[2 * a + 1];
    const double s = sin(phi + b), c = cos(phi + b);
    lm[0] = (T)(xv + r * c);                                              // (ekf.jl:99)
    lm[1] = (T)(yv + r * s);
    G[0][0] = 1.0; G[0][1] = 0.0; G[0][2] = -((double)lm[1] - l1);      // [I | J (lm - lin_xy)]
    G[1][0] = 0.0; G[1][1] = 1.0; G[1][2] = (double)lm[0] - l0;
    Gz[0][0] = c; Gz[0][1] = -r * s;                                      // (:103)
    Gz[1][0] = s; Gz[1][1] = r * c;
}

template <typename T>
__global__ __launch_bounds__(256) void fej_augment_kernel(T* __restrict__ x, T* __restrict__ P, int ld, int n0, const double* __restrict__ zn,
                                                           int nn, double R0, double R1, double R2, double R3,
                                                           const double* __restrict__ lin, double* __restrict__ first,
                                                           unsigned long long* __restrict__ pmax, int tlog, T* __restrict__ side, int side_n) {
    const double xv = (double)x[0], yv = (double)x[1], phi = (double)x[2];   // ekf.jl:88 (the pose is fixed for the call)
    const double l0 = lin[0], l1 = lin[1];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n0) {
        const double p0 = (double)P[p_off(ld, tlog, c, 0)];
        const double p1 = (double)P[p_off(ld, tlog, c, 1)];
        const double p2 = (double)P[p_off(ld, tlog, c, 2)];
        for (int a = 0; a < nn; ++a) {
            double G[2][3], Gz[2][2];
            T lm[2];
            fej_new_feature<T>(xv, yv, phi, l0, l1, zn, a, G, Gz, lm);
            const int fa = n0 + 2 * a;
            p_store_sym(P, ld, tlog, fa, c, (T)(p0 + G[0][2] * p2));      // P[fa, c] (:113, :117) and its mirror (:114, :118)
            p_store_sym(P, ld, tlog, fa + 1, c, (T)(p1 + G[1][2] * p2));
        }
    }
    if (blockIdx.x != 0) return;
    double Pvv[3][3];
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) Pvv[r][cc] = (double)P[p_off(ld, tlog, r, cc)];
    const double R[2][2] = {{R0, R2}, {R1, R3}};
    const int npairs = nn * (nn + 1) / 2;          // pairs (a, b) with b <= a
    for (int pidx = threadIdx.x; pidx < npairs; pidx += blockDim.x) {
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= pidx) ++a;
        const int b = pidx - a * (a + 1) / 2;
        double Ga[2][3], Gz[2][2], GaP[2][3];
        T lm[2];
        fej_new_feature<T>(xv, yv, phi, l0, l1, zn, a, Ga, Gz, lm);
        const int fa = n0 + 2 * a;
        for (int r = 0; r < 2; ++r)
            for (int cc = 0; cc < 3; ++cc) GaP[r][cc] = Ga[r][0] * Pvv[0][cc] + Ga[r][1] * Pvv[1][cc] + Ga[r][2] * Pvv[2][cc];
        if (a == b) {
            // P[rng, rng] = Gv Pvv Gv' + Gz R Gz' (:112): the lower triangle, each entry formed ONCE and stored with its mirror
            double GR[2][2];
            for (int r = 0; r < 2; ++r)
                for (int cc = 0; cc < 2; ++cc) GR[r][cc] = Gz[r][0] * R[0][cc] + Gz[r][1] * R[1][cc];
            for (int r = 0; r < 2; ++r)
                for (int cc = 0; cc <= r; ++cc) {
                    const double val = (GaP[r][0] * Ga[cc][0] + GaP[r][1] * Ga[cc][1] + GaP[r][2] * Ga[cc][2]) +
                                       (GR[r][0] * Gz[cc][0] + GR[r][1] * Gz[cc][1]);
                    p_store_sym(P, ld, tlog, fa + r, fa + cc, (T)val);
                    side_note(side, side_n, fa + r, fa + cc, (T)val);
                    if (r == cc) {       // the new variances enter the pre-gate's bound (ekf_gate.hip), as augment_kernel enters them
                        const double sv = (double)(T)val;
                        atomicMax(pmax, (unsigned long long)__double_as_longlong(sv >= 0.0 ? sv : __builtin_inf()));
                    }
                }
            x[fa] = lm[0];
            x[fa + 1] = lm[1];
            first[fa - 3] = (double)lm[0];
            first[fa - 2] = (double)lm[1];
        } else {
            // P[rng_a, rng_b] = Gv_a P[0:3, rng_b],  P[0:3, rng_b] = (Gv_b Pvv)'   (:114, :117 with rnm grown)
            double Gb[2][3], Gzb[2][2];
            T lmb[2];
            fej_new_feature<T>(xv, yv, phi, l0, l1, zn, b, Gb, Gzb, lmb);
            const int fb = n0 + 2 * b;
            for (int r = 0; r < 2; ++r)
                for (int cc = 0; cc < 2; ++cc)       // (Gv_a Pvv Gv_b')[r][cc]
                    p_store_sym(P, ld, tlog, fa + r, fb + cc, (T)(GaP[r][0] * Gb[cc][0] + GaP[r][1] * Gb[cc][1] + GaP[r][2] * Gb[cc][2]));
        }
    }
}

// ---- the linearisation points taken from x, renumbered, moved ------------------------------------------------------------------------
// first of landmark ids[t] (null: landmark t + 1) <- its stored mean, t < cnt; pose: lin <- the stored pose
template <typename T>
__global__ __launch_bounds__(256) void fej_take_kernel(const T* __restrict__ x, double* __restrict__ lin, double* __restrict__ first,
                                                        const int32_t* __restrict__ ids, int cnt, int pose) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (pose && t < 3) lin[t] = (double)x[t];
    if (t >= cnt) return;
    const int j = ids ? ids[t] - 1 : t;
    first[2 * j] = (double)x[3 + 2 * j];
    first[2 * j + 1] = (double)x[4 + 2 * j];
}

// dst of new landmark t + 1 <- src of old landmark ids[t], or the stored mean where ids[t] == 0
template <typename T>
__global__ __launch_bounds__(256) void fej_remap_kernel(const T* __restrict__ x, const double* __restrict__ src, double* __restrict__ dst,
                                                         const int32_t* __restrict__ ids, int cnt) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt) return;
    const int o = ids[t];
    dst[2 * t] = o ? src[2 * (o - 1)] : (double)x[3 + 2 * t];
    dst[2 * t + 1] = o ? src[2 * (o - 1) + 1] : (double)x[4 + 2 * t];
}

// p <- R p + t for lin's position and every first estimate, lin's heading wrapped once: thread 0 the pose, thread t >= 1 landmark t
__global__ __launch_bounds__(256) void fej_transform_kernel(double* __restrict__ lin, double* __restrict__ first, int N, double c, double s,
                                                            double tx, double ty, double theta) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > N) return;
    double* p = t == 0 ? lin : first + 2 * (t - 1);
    const double px = p[0], py = p[1];
    p[0] = c * px - s * py + tx;
    p[1] = s * px + c * py + ty;
    if (t == 0) lin[2] = mpi_to_pi_d(lin[2] + theta);
}

#define FEJ_SAME_MAP(f) ARG_CHECK((f)->N == (f)->h->N, "the map changed outside the object (its landmark count differs from the state's): call slam_ekf_fej_remap")

int take(slam_ekf_fej* f, const int32_t* ids_dev, int cnt, int pose) {
    slam_ekf* h = f->h;
    const dim3 grid(((cnt > 3 ? cnt : 3) + 255) / 256);
    if (h->dtype == SLAM_F32)
        hipLaunchKernelGGL(fej_take_kernel<float>, grid, dim3(256), 0, h->stream, (const float*)h->x, f->lin, f->first, ids_dev, cnt, pose);
    else
        hipLaunchKernelGGL(fej_take_kernel<double>, grid, dim3(256), 0, h->stream, (const double*)h->x, f->lin, f->first, ids_dev, cnt, pose);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

void release(slam_ekf_fej* f) {
    (void)hipFree(f->lin);
    (void)hipFree(f->first);
    (void)hipFree(f->spare);
    (void)hipFree(f->ids);
    delete f;
}

template <typename T>
int enqueue_update(slam_ekf_fej* f, int m) {
    slam_ekf* h = f->h;
    {
        KTimer t(h, SLAM_K_FACTOR);
        hipLaunchKernelGGL(fej_front_kernel<T>, dim3(1), dim3(256), 0, h->stream, (const T*)h->x, (const T*)h->P, h->ld, h->Smat, m,
                           (const double*)f->lin, (const double*)f->first, h->Cmat, h->gvec, h->d_small, h->d_status);
    }
    HIP_TRY(hipGetLastError());
    return enqueue_obs_panel<T>(h, m);
}

}  // namespace

extern "C" int slam_ekf_fej_create(slam_ekf_fej_t* out, slam_ekf_t h) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr, "null argument");
    *out = nullptr;
    ARG_CHECK(h != nullptr, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    slam_ekf_fej* f = new (std::nothrow) slam_ekf_fej();
    if (!f) {
        slam_set_error("out of host memory");
        return SLAM_E_NOMEM;
    }
    f->h = h;
    f->N = h->N;
    f->maxN = h->maxN;
    const size_t pts = sizeof(double) * 2 * (size_t)(h->maxN > 0 ? h->maxN : 1);
    int rc;
    if ((rc = slam_alloc_zero(&f->lin, sizeof(double) * 4, h->stream)) || (rc = slam_alloc_zero(&f->first, pts, h->stream)) ||
        (rc = slam_alloc_zero(&f->spare, pts, h->stream)) ||
        (rc = slam_alloc_zero(&f->ids, sizeof(int32_t) * (size_t)(h->maxN > 0 ? h->maxN : 1), h->stream)) ||
        (rc = take(f, nullptr, f->N, 1))) {
        (void)hipStreamSynchronize(h->stream);
        release(f);
        return rc;
    }
    *out = f;
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_destroy(slam_ekf_fej_t f) {
    SLAM_RANGE();
    if (!f) return SLAM_OK;
    (void)hipSetDevice(f->h->device);
    (void)hipStreamSynchronize(f->h->stream);                            // the last kernel that reads lin / first has run
    release(f);
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_predict(slam_ekf_fej_t f, double v, double g, double wheelbase, const double Q[4], double dt) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr && Q != nullptr, "null argument");
    const double vals[4] = {v, g, wheelbase, dt};
    ARG_CHECK(slam_all_finite(vals, 4) && slam_all_finite(Q, 4), "a value is not finite");
    FEJ_SAME_MAP(f);
    slam_ekf* h = f->h;
    HIP_TRY(hipSetDevice(h->device));
    const int n = 3 + 2 * h->N;
    const int blocks = h->N > 0 ? (2 * h->N + 255) / 256 : 1;
    int32_t* arrive = h->d_count + 3;                                     // predict_kernel's counter: one stream, left at zero
    {
        KTimer t(h, SLAM_K_PREDICT);
        if (h->dtype == SLAM_F32)
            hipLaunchKernelGGL(fej_strip_kernel<float>, dim3(blocks), dim3(256), 0, h->stream, (float*)h->x, (float*)h->P, h->ld, n, f->lin, v,
                               g, wheelbase, Q[0], Q[1], Q[2], Q[3], dt, arrive, 7);
        else
            hipLaunchKernelGGL(fej_strip_kernel<double>, dim3(blocks), dim3(256), 0, h->stream, (double*)h->x, (double*)h->P, h->ld, n, f->lin,
                               v, g, wheelbase, Q[0], Q[1], Q[2], Q[3], dt, arrive, 6);
    }
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_update(slam_ekf_fej_t f, const double* zf, const int32_t* idf, int m, const double R[4], double out[4]) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr, "null handle");
    ARG_CHECK(zf != nullptr && idf != nullptr && R != nullptr && out != nullptr, "null argument");
    ARG_CHECK(m >= 1 && m <= SLAM_FEJ_MAXOBS, "m outside 1 .. SLAM_FEJ_MAXOBS");
    ARG_CHECK(slam_all_finite(zf, 2 * m), "zf is not finite");
    int rc;
    if ((rc = check_R(R))) return rc;
    FEJ_SAME_MAP(f);
    slam_ekf* h = f->h;
    std::vector<double> blob;
    if ((rc = obs_block_fill(h, zf, idf, m, R, blob))) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = ensure_update_workspace(h, MO))) return rc;                 // kcap >= 32: Smat holds the block, W1 16 columns
    SlamDrainOnExit drain{h->stream};
    HIP_TRY(hipMemcpyAsync(h->Smat, blob.data(), sizeof(double) * B_IN, hipMemcpyHostToDevice, h->stream));
    rc = h->dtype == SLAM_F32 ? enqueue_update<float>(f, m) : enqueue_update<double>(f, m);
    if (rc) return rc;
    h->grid_force = 1;                                                    // the means moved: the grid is rebuilt at the next query
    if ((rc = slam_small_out(h, out, 4, 3)) == SLAM_E_NOTPD)
        slam_set_error("FEJ update: S is not positive definite, pivot %d is %g (state left unchanged)", (int)out[3], out[2]);
    return rc;
}

extern "C" int slam_ekf_fej_augment(slam_ekf_fej_t f, const double* zn, int cnt, const double R[4]) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr, "null handle");
    ARG_CHECK(cnt >= 0, "cnt < 0");
    if (cnt == 0) return SLAM_OK;
    ARG_CHECK(zn != nullptr && R != nullptr, "null argument");
    ARG_CHECK(slam_all_finite(zn, 2 * cnt), "zn is not finite");
    int rc;
    if ((rc = check_R(R))) return rc;
    FEJ_SAME_MAP(f);
    slam_ekf* h = f->h;
    if (h->N + cnt > h->maxN || h->N + cnt > f->maxN) {
        slam_set_error("augment: %d + %d landmarks exceed capacity %d", h->N, cnt, h->maxN < f->maxN ? h->maxN : f->maxN);
        return SLAM_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(h->device));
    // the observations go through the handle's pinned staging buffer, as slam_ekf_augment stages them: enqueued, no synchronise
    if ((rc = ensure_obs_capacity(h, cnt))) return rc;
    if (h->stage_pending) {                                               // (it may still be the source of an earlier copy)
        HIP_TRY(hipEventSynchronize(h->stage_ev));
        h->stage_pending = 0;
    }
    memcpy(h->h_obs, zn, sizeof(double) * 2 * (size_t)cnt);
    HIP_TRY(hipMemcpyAsync(h->obsbuf, h->h_obs, sizeof(double) * 2 * (size_t)cnt, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipEventRecord(h->stage_ev, h->stream));
    h->stage_pending = 1;
    const int n0 = 3 + 2 * h->N;
    const int blocks = (n0 + 255) / 256;
    {
        KTimer t(h, SLAM_K_AUGMENT);
        if (h->dtype == SLAM_F32)
            hipLaunchKernelGGL(fej_augment_kernel<float>, dim3(blocks), dim3(256), 0, h->stream, (float*)h->x, (float*)h->P, h->ld, n0,
                               (const double*)h->obsbuf, cnt, R[0], R[1], R[2], R[3], (const double*)f->lin, f->first,
                               (unsigned long long*)h->d_pmax, 7, (float*)h->Pside, h->npad / 2);
        else
            hipLaunchKernelGGL(fej_augment_kernel<double>, dim3(blocks), dim3(256), 0, h->stream, (double*)h->x, (double*)h->P, h->ld, n0,
                               (const double*)h->obsbuf, cnt, R[0], R[1], R[2], R[3], (const double*)f->lin, f->first,
                               (unsigned long long*)h->d_pmax, 6, (double*)h->Pside, h->npad / 2);
    }
    HIP_TRY(hipGetLastError());
    h->N += cnt;
    f->N += cnt;
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_reset(slam_ekf_fej_t f, const int32_t* ids, int cnt, int pose) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr, "null handle");
    ARG_CHECK(cnt >= -1, "cnt < -1");
    ARG_CHECK(cnt <= 0 || ids != nullptr, "null argument");
    FEJ_SAME_MAP(f);
    ARG_CHECK(cnt <= f->N, "more ids than landmarks");
    for (int t = 0; t < cnt; ++t) ARG_CHECK(ids[t] >= 1 && ids[t] <= f->N, "landmark id out of range");
    slam_ekf* h = f->h;
    HIP_TRY(hipSetDevice(h->device));
    if (cnt < 0) return take(f, nullptr, f->N, pose);
    SlamDrainOnExit drain{h->stream};
    if (cnt > 0) HIP_TRY(hipMemcpyAsync(f->ids, ids, sizeof(int32_t) * (size_t)cnt, hipMemcpyHostToDevice, h->stream));
    return take(f, f->ids, cnt, pose);
}

extern "C" int slam_ekf_fej_remap(slam_ekf_fej_t f, const int32_t* ids, int cnt) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr, "null handle");
    slam_ekf* h = f->h;
    ARG_CHECK(cnt == h->N, "cnt must be the state's landmark count");
    ARG_CHECK(cnt <= f->maxN, "the state's map is larger than the object's capacity");
    ARG_CHECK(cnt == 0 || ids != nullptr, "null argument");
    for (int t = 0; t < cnt; ++t) ARG_CHECK(ids[t] >= 0 && ids[t] <= f->N, "landmark id out of range");
    HIP_TRY(hipSetDevice(h->device));
    if (cnt > 0) {
        SlamDrainOnExit drain{h->stream};
        HIP_TRY(hipMemcpyAsync(f->ids, ids, sizeof(int32_t) * (size_t)cnt, hipMemcpyHostToDevice, h->stream));
        const dim3 grid((cnt + 255) / 256);
        if (h->dtype == SLAM_F32)
            hipLaunchKernelGGL(fej_remap_kernel<float>, grid, dim3(256), 0, h->stream, (const float*)h->x, (const double*)f->first, f->spare,
                               (const int32_t*)f->ids, cnt);
        else
            hipLaunchKernelGGL(fej_remap_kernel<double>, grid, dim3(256), 0, h->stream, (const double*)h->x, (const double*)f->first, f->spare,
                               (const int32_t*)f->ids, cnt);
        HIP_TRY(hipGetLastError());
        double* t = f->first;
        f->first = f->spare;
        f->spare = t;
    }
    f->N = cnt;
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_transform(slam_ekf_fej_t f, double tx, double ty, double theta) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr, "null handle");
    ARG_CHECK(std::isfinite(tx) && std::isfinite(ty) && std::isfinite(theta), "tx, ty and theta must be finite");
    FEJ_SAME_MAP(f);
    theta = remainder(theta, 2.0 * SLAM_PI_D);                            // as slam_ekf_transform reduces it
    const double c = cos(theta), s = sin(theta);
    HIP_TRY(hipSetDevice(f->h->device));
    hipLaunchKernelGGL(fej_transform_kernel, dim3((f->N + 1 + 255) / 256), dim3(256), 0, f->h->stream, f->lin, f->first, f->N, c, s, tx, ty, theta);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_get(slam_ekf_fej_t f, double lin[3], double* first, int32_t* count) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr, "null handle");
    HIP_TRY(hipSetDevice(f->h->device));
    SlamDrainOnExit drain{f->h->stream};
    if (lin) HIP_TRY(hipMemcpyAsync(lin, f->lin, sizeof(double) * 3, hipMemcpyDeviceToHost, f->h->stream));
    if (first && f->N > 0) HIP_TRY(hipMemcpyAsync(first, f->first, sizeof(double) * 2 * (size_t)f->N, hipMemcpyDeviceToHost, f->h->stream));
    if (count) *count = f->N;
    HIP_TRY(hipStreamSynchronize(f->h->stream));
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_set(slam_ekf_fej_t f, const double lin[3], const double* first) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr, "null handle");
    slam_ekf* h = f->h;
    ARG_CHECK(!lin || slam_all_finite(lin, 3), "lin is not finite");
    ARG_CHECK(!first || h->N <= f->maxN, "the state's map is larger than the object's capacity");
    ARG_CHECK(!first || slam_all_finite(first, 2 * h->N), "first is not finite");
    ARG_CHECK(first || f->N == h->N, "the map changed outside the object: first must be given");
    HIP_TRY(hipSetDevice(h->device));
    SlamDrainOnExit drain{h->stream};
    if (lin) HIP_TRY(hipMemcpyAsync(f->lin, lin, sizeof(double) * 3, hipMemcpyHostToDevice, h->stream));
    if (first) {
        if (h->N > 0) HIP_TRY(hipMemcpyAsync(f->first, first, sizeof(double) * 2 * (size_t)h->N, hipMemcpyHostToDevice, h->stream));
        f->N = h->N;
    }
    return SLAM_OK;
}

extern "C" int slam_ekf_fej_limits(int32_t out[1]) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr, "null argument");
    out[0] = SLAM_FEJ_MAXOBS;
    return SLAM_OK;
}
