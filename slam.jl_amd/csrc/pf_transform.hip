// pf_transform.hip -- the FastSLAM state expressed in another frame (slam_pf_transform): every particle's pose and every
// landmark record IN USE through p <- R p + t, phi <- wrap_pi(phi + theta), Pf <- R Pf R'.  Elementwise: one pass over the live
// pose buffer [3][n] and one over the records [nl][5][n] of buffer `cur` (chunk by chunk through LmView), both bound by HBM
// (24 / 40 bytes per pose and 40 / 80 bytes per record, read + write, fp32 / fp64).  The log-weights, the RNG step, `seen`
// and the resampling count are not touched.  R = [c -s; s c] comes from the host; everything is evaluated in double from the
// stored values and rounded once.
#include <cfloat>
#include <cmath>

#include "pf_device.h"
#include "../../include/slamhip_frame.h"

namespace {

constexpr int XF_PER = 4;                   // particles per thread (strided by the workgroup: every load is coalesced)
constexpr int XF_LMS = 2048;                // landmarks per launch: their `seen` bits travel as a kernel argument
struct XfSeen { unsigned long long w[XF_LMS / 64]; };

template <typename T>
__global__ __launch_bounds__(256) void pf_transform_pose_kernel(T* __restrict__ pose, int64_t n, double c, double s, double tx, double ty,
                                                                 double theta) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const double x = (double)pose[p], y = (double)pose[n + p];
    pose[p] = (T)(c * x - s * y + tx);
    pose[n + p] = (T)(s * x + c * y + ty);
    pose[2 * n + p] = wrap_pi<T>((T)((double)pose[2 * n + p] + theta));
}

// grid (slabs of 256 * XF_PER particles, landmarks l0 .. l0 + gridDim.y).  A record is in use as pf_map.hip reads it: Pxx > 0, or
// Pxx == 0 with the landmark `seen`; the empty slot (Pxx = -1) and the never-seen all-zero record are not written at all.
// Pxx is the in-use mark as well: a record that had Pxx > 0 keeps a positive one (the smallest normal number when the
// rotated value rounds to zero or below: a rank-one covariance turned onto the y axis).
template <typename T>
__global__ __launch_bounds__(256) void pf_transform_lm_kernel(LmView<T> lv, int buf, int64_t n, int l0, XfSeen seen, double c, double s,
                                                               double tx, double ty) {
    const int ly = blockIdx.y;
    const bool sn = (seen.w[ly >> 6] >> (ly & 63)) & 1ull;
    T* __restrict__ rows = lv.rows(buf, l0 + ly, n);
    const double cc = c * c, ss = s * s, cs = c * s;
    T v[XF_PER][5];
#pragma unroll
    for (int j = 0; j < XF_PER; ++j) {
        const int64_t p = ((int64_t)blockIdx.x * XF_PER + j) * 256 + threadIdx.x;
        if (p < n) {
#pragma unroll
            for (int k = 0; k < 5; ++k) v[j][k] = rows[(size_t)k * (size_t)n + p];
        } else {
            v[j][2] = (T)-1;
        }
    }
#pragma unroll
    for (int j = 0; j < XF_PER; ++j) {
        const int64_t p = ((int64_t)blockIdx.x * XF_PER + j) * 256 + threadIdx.x;
        const T pxx0 = v[j][2];
        if (p >= n || !(pxx0 > (T)0 || (sn && pxx0 == (T)0))) continue;
        const double mx = (double)v[j][0], my = (double)v[j][1], pxx = (double)pxx0, pxy = (double)v[j][3], pyy = (double)v[j][4];
        T qxx = (T)(cc * pxx - 2.0 * cs * pxy + ss * pyy);
        if (pxx0 > (T)0 && !(qxx > (T)0)) qxx = sizeof(T) == 4 ? (T)FLT_MIN : (T)DBL_MIN;
        rows[p] = (T)(c * mx - s * my + tx);
        rows[(size_t)n + p] = (T)(s * mx + c * my + ty);
        rows[2 * (size_t)n + p] = qxx;
        rows[3 * (size_t)n + p] = (T)(cs * (pxx - pyy) + (cc - ss) * pxy);
        rows[4 * (size_t)n + p] = (T)(ss * pxx + 2.0 * cs * pxy + cc * pyy);
    }
}

}  // namespace

/* slamhip_frame.h: the rigid frame change (tx, ty, theta) of every pose and every landmark record in use.  Begins as
 * slam_pf_step_unknown does; enqueued. */
extern "C" int slam_pf_transform(slam_pf_t h, double tx, double ty, double theta) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK(std::isfinite(tx) && std::isfinite(ty) && std::isfinite(theta), "tx, ty and theta must be finite");
    theta = remainder(theta, 2.0 * PF_PI);
    const double c = cos(theta), s = sin(theta);
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    int rc;
    if ((rc = pf_flush_pending(h))) return rc;                // a deferred normalisation shift, as slam_pf_download honours it
    if ((rc = pf_materialise(h))) return rc;                  // every record to (buffer cur, its particle's slot); collective with peers
    const int64_t n = h->n;
    PF_DISPATCH(h,
                hipLaunchKernelGGL(pf_transform_pose_kernel<T>, dim3(grid_for(n)), dim3(256), 0, h->stream, (T*)h->pose[h->pcur], n, c, s,
                                   tx, ty, theta),
                hipLaunchKernelGGL(pf_transform_pose_kernel<T>, dim3(grid_for(n)), dim3(256), 0, h->stream, (T*)h->pose[h->pcur], n, c, s,
                                   tx, ty, theta));
    HIP_TRY(hipGetLastError());
    const int slabs = (int)((n + 256 * XF_PER - 1) / (256 * XF_PER));
    for (int l0 = 0; l0 < h->nl; l0 += XF_LMS) {
        const int cnt = h->nl - l0 < XF_LMS ? h->nl - l0 : XF_LMS;
        XfSeen seen;
        memset(&seen, 0, sizeof(seen));
        for (int i = 0; i < cnt; ++i)
            if (h->seen[l0 + i]) seen.w[i >> 6] |= 1ull << (i & 63);
        PF_DISPATCH(h,
                    hipLaunchKernelGGL(pf_transform_lm_kernel<T>, dim3(slabs, cnt), dim3(256), 0, h->stream, LmView<T>{h->d_lmtab}, h->cur,
                                       n, l0, seen, c, s, tx, ty),
                    hipLaunchKernelGGL(pf_transform_lm_kernel<T>, dim3(slabs, cnt), dim3(256), 0, h->stream, LmView<T>{h->d_lmtab}, h->cur,
                                       n, l0, seen, c, s, tx, ty));
        HIP_TRY(hipGetLastError());
    }
    return SLAM_OK;
}
