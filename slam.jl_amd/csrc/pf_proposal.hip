// pf_proposal.hip -- FastSLAM 2.0 with UNKNOWN correspondences (include/ext/slamhip_proposal.h, which states the rule):
// per-particle association under the prior proposal, the observation-aware proposal over the matched observations, the draw,
// the map updates from the sampled pose and the weight statistics in ONE launch.  libslamhip_proposal.so.
//
// One particle per lane, 256-particle workgroups (the unit of the weight statistics: block_weight_stats and the fold must see
// the blocks pf_stats_kernel sees for the three numbers to come out bit for bit); idle lanes of the last workgroup shadow
// particle n - 1 and every store is masked.  At most 16 observations: the 16 running minima and the decisions stay in the
// lane's registers (every loop over the observations is unrolled, nothing is indexed with a run-time observation number).
//
//   pass A  sweeps the slots ONCE through the sweep's buffer descriptors (lm_rsrc / rec_load, own slot of buffer `cur`: the
//           host materialises first); the next record is requested before the current one is scored.  Per slot: the quantities
//           that do not depend on the observation at the MEAN pose with the pose term B B' in S, then the 16 scores.  The
//           arithmetic is pf_update_unknown_kernel's (exact sqrt / atan2 / log / divisions in fp32 too) plus B = Hv GL.
//   pass B  re-reads the at most m MATCHED records (the lane's own decision: a per-lane slot, plain loads, PF_DEPTH in flight)
//           and runs the proposal.  The per-observation body is proposal_core's (pf_device.h), copied term for term with the
//           landmark taken from the lane's decision instead of a staged id; pf_device.h itself is untouched, so the product
//           kernels keep their instructions.
//   pass C  the draw (normals2 / motion_pose), then the updates in observation order as pf_update_unknown_kernel's second pass
//           applies them: lm_update on the matched slot, lm_init in the lowest unused slot, -2 when none is left.
//   stats   block_weight_stats, the partial record pf_stats_kernel writes.
//
// A decision < 0 never becomes a record index: every use of a decision as a slot is behind `a >= 0` (and a < nl by
// construction: pass A only ever stores its loop counter).
#include <cmath>

#include "pf_device.h"
#include "../../include/ext/slamhip_proposal.h"

namespace {

constexpr int PU_MAX = SLAM_PF_PROPOSAL_MAXOBS;      // observations per lane
constexpr int PU_WG = 256;                           // particles per workgroup

// mean motion and GL = Gu Lq (proposal_core, pf_device.h)
template <typename T>
struct PuMean {
    T xm, ym, pm, gl00, gl01, gl10, gl11, gl20, gl21;
};
template <typename T>
__device__ __forceinline__ PuMean<T> pu_mean(T x, T y, T phi, T V, T G, T wheelbase, T lq00, T lq10, T lq11, T dt) {
    T s, c, sG, cG;
    m_sincos<T>(G + phi, s, c);
    m_sincos<T>(G, sG, cG);
    const T vts = V * dt * s, vtc = V * dt * c;
    PuMean<T> q;
    q.xm = x + vtc; q.ym = y + vts;
    q.pm = wrap_pi<T>(phi + V * dt * sG / wheelbase);
    const T gu20 = dt * sG / wheelbase, gu21 = V * dt * cG / wheelbase;
    q.gl00 = dt * c * lq00 + (-vts) * lq10; q.gl01 = (-vts) * lq11;
    q.gl10 = dt * s * lq00 + vtc * lq10; q.gl11 = vtc * lq11;
    q.gl20 = gu20 * lq00 + gu21 * lq10; q.gl21 = gu21 * lq11;
    return q;
}

// pass A: decisions of the lane's m observations against the map of particle p (buffer buf, own slots), at the mean pose.
// NIS: also keep the nis of the running winner.
template <typename T, bool NIS>
__device__ __forceinline__ void pu_associate(const LmView<T> lv, int buf, int64_t n, int64_t p, int nl, const PuMean<T>& q,
                                             const double* s_obs, int m, T R00, T R10, T R01, T R11, T gate1, T gate2,
                                             int (&dec)[PU_MAX], T (&win)[NIS ? PU_MAX : 1]) {
    const T INF = (T)__builtin_inf();
    T best_nd[PU_MAX];
    int best_l[PU_MAX];
    unsigned near = 0u;
#pragma unroll
    for (int i = 0; i < PU_MAX; ++i) { best_nd[i] = INF; best_l[i] = -1; }
    if constexpr (NIS) {
#pragma unroll
        for (int i = 0; i < PU_MAX; ++i) win[i] = (T)__builtin_nan("");
    }
    // Records are read through the sweep's buffer descriptors (lm_rsrc: the landmark's five rows, the field's row as the scalar
    // offset, the lane's slot as the vector offset).  Pxx decides whether a slot holds a landmark, so it runs TWO slots ahead
    // and the other four rows ONE slot ahead, only in the lanes whose slot is in use: a half-empty map costs 4 B per unused slot
    // and particle, not 20.  (Default cache policy: passes B and C read the matched records again.)
    const uint32_t voff = (uint32_t)p * (uint32_t)sizeof(T), row = (uint32_t)n * (uint32_t)sizeof(T);
    auto pxx_of = [&](int l) { return rec_load<T, 0>(lm_rsrc<T>(lv.rows(buf, l, n), n), voff, 2u * row); };
    auto rest_of = [&](int l, T pxx) {
        LmRow<T> r{0, 0, pxx, 0, 0};
        if (!(pxx < (T)0)) {
            const auto rs = lm_rsrc<T>(lv.rows(buf, l, n), n);
            r.lx = rec_load<T, 0>(rs, voff, 0u);
            r.ly = rec_load<T, 0>(rs, voff, row);
            r.pxy = rec_load<T, 0>(rs, voff, 3u * row);
            r.pyy = rec_load<T, 0>(rs, voff, 4u * row);
        }
        return r;
    };
    LmRow<T> nxt{0, 0, (T)-1, 0, 0};
    T pn = (T)-1;                                        // Pxx of slot l + 1
    if (nl > 0) {
        const T p0 = pxx_of(0);
        if (nl > 1) pn = pxx_of(1);
        nxt = rest_of(0, p0);
    }
    for (int l = 0; l < nl; ++l) {
        const LmRow<T> cur = nxt;
        T pnn = (T)-1;
        if (l + 2 < nl) pnn = pxx_of(l + 2);
        nxt = rest_of(l + 1 < nl ? l + 1 : l, l + 1 < nl ? pn : (T)-1);
        pn = pnn;
        if (cur.pxx < (T)0) continue;
        const T dx = cur.lx - q.xm, dy = cur.ly - q.ym;
        const T d2 = dx * dx + dy * dy;
        const T d = sqrt(d2);
        const T zp1 = atan2(dy, dx) - q.pm;
        const T h00 = dx / d, h01 = dy / d, h10 = -dy / d2, h11 = dx / d2;      // src/common.jl:162
        const T t00 = cur.pxx * h00 + cur.pxy * h01, t01 = cur.pxx * h10 + cur.pxy * h11;
        const T t10 = cur.pxy * h00 + cur.pyy * h01, t11 = cur.pxy * h10 + cur.pyy * h11;
        T s00 = h00 * t00 + h01 * t10 + R00;                                    // Hf Pf Hf' + R, not symmetrised
        T s01 = h00 * t01 + h01 * t11 + R01;
        T s10 = h10 * t00 + h11 * t10 + R10;
        T s11 = h10 * t01 + h11 * t11 + R11;
        // B = Hv GL with Hv = [-h00 -h01 0; -h10 -h11 -1]  (src/common.jl:161)
        const T b00 = -(h00 * q.gl00 + h01 * q.gl10), b01 = -(h00 * q.gl01 + h01 * q.gl11);
        const T b10 = -(h10 * q.gl00 + h11 * q.gl10) - q.gl20, b11 = -(h10 * q.gl01 + h11 * q.gl11) - q.gl21;
        s00 = s00 + (b00 * b00 + b01 * b01);                                    // + B B': the pose term (Sigma = I)
        s01 = s01 + (b00 * b10 + b01 * b11);
        s10 = s10 + (b10 * b00 + b11 * b01);
        s11 = s11 + (b10 * b10 + b11 * b11);
        const T det = s00 * s11 - s01 * s10;
        const T rdet = (T)1 / det;
        const T qa = s11 * rdet, qb = -(s01 + s10) * rdet, qc = s00 * rdet;
        const T logdet = log(det);
#pragma unroll
        for (int i = 0; i < PU_MAX; ++i) {
            if (i < m) {
                const T v0 = (T)s_obs[2 * i] - d;
                const T v1 = wrap_pi<T>((T)s_obs[2 * i + 1] - zp1);
                const T nis = qa * v0 * v0 + qb * v0 * v1 + qc * v1 * v1;
                const T nd = nis + logdet;
                if (nis < gate1 && nd < best_nd[i]) {                            // strict: the lowest slot wins a tie
                    best_nd[i] = nd;
                    best_l[i] = l;
                    if constexpr (NIS) win[i] = nis;
                }
                if (nis <= gate2) near |= 1u << i;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PU_MAX; ++i) dec[i] = best_l[i] >= 0 ? best_l[i] : (((near >> i) & 1u) ? -2 : -1);
}

// the record of slot a of particle p; a is a slot (0 <= a < nl): the caller has checked
template <typename T>
__device__ __forceinline__ LmRow<T> pu_row(const LmView<T> lv, int buf, int a, int64_t n, int64_t p) {
    return load_row<T>(lv.rows(buf, a, n) + p, n);
}

template <typename T>
__global__ __launch_bounds__(PU_WG) void pf_proposal_unknown_kernel(
    T* __restrict__ pose, LmView<T> lv, int buf, T* __restrict__ logw, int64_t n, int64_t first, uint32_t step, uint64_t seed,
    T V, T G, T wheelbase, T lq00, T lq10, T lq11, T dt, int nl, const double* __restrict__ z, int m, T R00, T R10, T R01, T R11,
    T gate1, T gate2, T pend, int32_t* __restrict__ assoc_out, double* __restrict__ part) {
    __shared__ double s_obs[2 * PU_MAX];
    if (m > PU_MAX) m = PU_MAX;                          // (the host has refused it)
    for (int i = threadIdx.x; i < 2 * m; i += blockDim.x) s_obs[i] = z[i];
    __syncthreads();
    const int64_t pi = (int64_t)blockIdx.x * PU_WG + threadIdx.x;
    const bool valid = pi < n;
    const int64_t p = valid ? pi : n - 1;                // idle lanes shadow the last particle, stores are masked
    const T x = pose[p], y = pose[n + p], phi = pose[2 * n + p];
    T lw = logw[p] - pend;
    const PuMean<T> q = pu_mean<T>(x, y, phi, V, G, wheelbase, lq00, lq10, lq11, dt);

    // ---- pass A
    int dec[PU_MAX];
    T unused_nis[1];
    pu_associate<T, false>(lv, buf, n, p, nl, q, s_obs, m, R00, R10, R01, R11, gate1, gate2, dec, unused_nis);

    // ---- pass B: the proposal over the matched observations, every record read from the PRIOR map
    T mu0 = 0, mu1 = 0, g00 = 1, g01 = 0, g11 = 1;
    {
        const T xm = q.xm, ym = q.ym, pm = q.pm;
        const T gl00 = q.gl00, gl01 = q.gl01, gl10 = q.gl10, gl11 = q.gl11, gl20 = q.gl20, gl21 = q.gl21;
        LmRow<T> ring[PF_DEPTH];
#pragma unroll
        for (int u = 0; u < PF_DEPTH; ++u) {
            ring[u] = LmRow<T>{0, 0, 0, 0, 0};
            if (u < m && dec[u] >= 0) ring[u] = pu_row<T>(lv, buf, dec[u], n, p);
        }
#pragma unroll
        for (int i = 0; i < PU_MAX; ++i) {
            if (i < m) {                                   // uniform
                constexpr int PD = PF_DEPTH;
                const LmRow<T> cur = ring[i % PD];
                if (i + PD < PU_MAX) {
                    const int j = i + PD < PU_MAX ? i + PD : PU_MAX - 1;
                    if (j < m && dec[j] >= 0) ring[i % PD] = pu_row<T>(lv, buf, dec[j], n, p);
                }
                if (dec[i] >= 0) {
                    // (proposal_core's per-observation body, pf_device.h, term for term)
                    const T r = (T)s_obs[2 * i], b = (T)s_obs[2 * i + 1];
                    const T dx = cur.lx - xm, dy = cur.ly - ym;
                    const T d2 = dx * dx + dy * dy;
                    T d, h00, h01, h10, h11;
                    if constexpr (sizeof(T) == 4) {
                        const T rd = __builtin_amdgcn_rsqf(d2);
                        d = d2 * rd;
                        const T rd2 = rd * rd;
                        h00 = dx * rd; h01 = dy * rd; h10 = -dy * rd2; h11 = dx * rd2;           // src/common.jl:162
                    } else {
                        d = sqrt(d2);
                        h00 = dx / d; h01 = dy / d; h10 = -dy / d2; h11 = dx / d2;
                    }
                    // B = Hv GL with Hv = [-h00 -h01 0; -h10 -h11 -1]  (src/common.jl:161)
                    const T b00 = -(h00 * gl00 + h01 * gl10), b01 = -(h00 * gl01 + h01 * gl11);
                    const T b10 = -(h10 * gl00 + h11 * gl10) - gl20, b11 = -(h10 * gl01 + h11 * gl11) - gl21;
                    const T v0 = (r - d) - (b00 * mu0 + b01 * mu1);
                    const T v1 = wrap_pi<T>(b - (m_atan2<T>(dy, dx) - pm)) - (b10 * mu0 + b11 * mu1);
                    const T t00 = cur.pxx * h00 + cur.pxy * h01, t01 = cur.pxx * h10 + cur.pxy * h11;      // Pf Hf'
                    const T t10 = cur.pxy * h00 + cur.pyy * h01, t11 = cur.pxy * h10 + cur.pyy * h11;
                    const T f00 = h00 * t00 + h01 * t10 + R00;                                            // Sf, symmetrised
                    const T f01 = (T)0.5 * ((h00 * t01 + h01 * t11 + R01) + (h10 * t00 + h11 * t10 + R10));
                    const T f11 = h10 * t01 + h11 * t11 + R11;
                    const T q00 = g00 * b00 + g01 * b01, q01 = g00 * b10 + g01 * b11;                       // Sig B'
                    const T q10 = g01 * b00 + g11 * b01, q11 = g01 * b10 + g11 * b11;
                    const T s00 = b00 * q00 + b01 * q10 + f00;                                            // S = B Sig B' + Sf
                    const T s01 = (T)0.5 * ((b00 * q01 + b01 * q11 + f01) + (b10 * q00 + b11 * q10 + f01));
                    const T s11 = b10 * q01 + b11 * q11 + f11;
                    T u00, u01, u11, c00, c01, c11;                                                       // chol(S) upper, C = inv(U)
                    if constexpr (sizeof(T) == 4) {
                        c00 = __builtin_amdgcn_rsqf(s00);
                        u00 = s00 * c00;
                        u01 = s01 * c00;
                        const T tt = s11 - u01 * u01;
                        c11 = __builtin_amdgcn_rsqf(tt);
                        u11 = tt * c11;
                        c01 = -u01 * (c00 * c11);
                    } else {
                        u00 = sqrt(s00);
                        u01 = s01 / u00;
                        u11 = sqrt(s11 - u01 * u01);
                        c00 = (T)1 / u00; c01 = -u01 / (u00 * u11); c11 = (T)1 / u11;
                    }
                    const T w00 = q00 * c00, w01 = q00 * c01 + q01 * c11;
                    const T w10 = q10 * c00, w11 = q10 * c01 + q11 * c11;
                    const T y0 = c00 * v0, y1 = c01 * v0 + c11 * v1;
                    mu0 = mu0 + (w00 * y0 + w01 * y1);
                    mu1 = mu1 + (w10 * y0 + w11 * y1);
                    g00 = g00 - (w00 * w00 + w01 * w01);
                    g01 = g01 - (w00 * w10 + w01 * w11);
                    g11 = g11 - (w10 * w10 + w11 * w11);
                    // the guard of proposal_core: Sig is kept positive semi-definite, a positive definite Sig keeps its bits
                    g00 = fmax(g00, (T)0);
                    g11 = fmax(g11, (T)0);
                    if constexpr (kFast<T>) {
                        const T glim = m_sqrt<T>(g00 * g11);
                        g01 = fmin(fmax(g01, -glim), glim);
                    } else {
                        const T gdet = g00 * g11;
                        if (g01 * g01 > gdet) g01 = copysign(sqrt(gdet), g01);
                    }
                    lw += (T)-0.5 * (y0 * y0 + y1 * y1) - m_log<T>(u00 * u11) - (T)1.8378770664093453;
                }
            }
        }
    }

    // ---- the draw: w ~ N(mu, Sig), the control, the pose (proposal_core)
    T e1, e2;
    normals2<T>((uint64_t)(first + p), step, STREAM_PREDICT, seed, e1, e2);
    const T l00 = sqrt(g00);
    const T l10 = l00 > (T)0 ? g01 / l00 : (T)0;
    const T l11 = sqrt(fmax(g11 - l10 * l10, (T)0));
    const T w0 = mu0 + l00 * e1;
    const T w1 = mu1 + l10 * e1 + l11 * e2;
    const T Vn = V + lq00 * w0;
    const T Gn = G + (lq10 * w0 + lq11 * w1);
    const PfPose<T> qs = motion_pose<T, T>(Vn, Gn, dt, wheelbase, x, y, phi, valid, pose, n, p);
    const T xn = qs.x, yn = qs.y, pn = qs.phi;
    if (valid) logw[p] = lw;

    // ---- pass C: the updates in observation order from the sampled pose; the weight is left alone
    T lw_unused = 0;
    int next_free = 0;                                   // unused slots are handed out in ascending order
#pragma unroll
    for (int i = 0; i < PU_MAX; ++i) {
        if (i < m) {
            int a = dec[i];
            const T r = (T)s_obs[2 * i], b = (T)s_obs[2 * i + 1];
            if (a >= 0) {
                T* row = lv.rows(buf, a, n) + p;
                const LmRow<T> cur = load_row<T>(row, n);
                lm_update<T>(row, n, cur, xn, yn, pn, r, b, R00, R10, R01, R11, valid, lw_unused);
            } else if (a == -1) {
                int slot = next_free;
                while (slot < nl && !(lv.rows(buf, slot, n)[2 * n + p] < (T)0)) ++slot;
                if (slot < nl) {
                    lm_init<T>(lv.rows(buf, slot, n) + p, n, xn, yn, pn, r, b, R00, R10, R01, R11, valid);
                    next_free = slot + 1;
                } else {
                    next_free = nl;
                    a = -2;                              // no slot left: dropped
                }
            }
            if (assoc_out && valid) assoc_out[(size_t)i * n + p] = a;
        }
    }
    block_weight_stats<T, false, false>(lw, xn, yn, pn, valid, 1, part);
}

template <typename T>
__global__ __launch_bounds__(PU_WG) void pf_associate_proposal_kernel(
    const T* __restrict__ pose, LmView<T> lv, int buf, int64_t n, T V, T G, T wheelbase, T lq00, T lq10, T lq11, T dt, int nl,
    const double* __restrict__ z, int m, T R00, T R10, T R01, T R11, T gate1, T gate2, int32_t* __restrict__ assoc_out,
    T* __restrict__ nis_out) {
    __shared__ double s_obs[2 * PU_MAX];
    if (m > PU_MAX) m = PU_MAX;
    for (int i = threadIdx.x; i < 2 * m; i += blockDim.x) s_obs[i] = z[i];
    __syncthreads();
    const int64_t pi = (int64_t)blockIdx.x * PU_WG + threadIdx.x;
    const bool valid = pi < n;
    const int64_t p = valid ? pi : n - 1;
    const PuMean<T> q = pu_mean<T>(pose[p], pose[n + p], pose[2 * n + p], V, G, wheelbase, lq00, lq10, lq11, dt);
    int dec[PU_MAX];
    T win[PU_MAX];
    pu_associate<T, true>(lv, buf, n, p, nl, q, s_obs, m, R00, R10, R01, R11, gate1, gate2, dec, win);
#pragma unroll
    for (int i = 0; i < PU_MAX; ++i) {
        if (i < m && valid) {
            if (assoc_out) assoc_out[(size_t)i * n + p] = dec[i];
            if (nis_out) nis_out[(size_t)i * n + p] = win[i];
        }
    }
}

struct PuArgs {
    double lq00, lq10, lq11, R[4];
};

// the argument rules of the header; nothing is enqueued and nothing of the handle is written
int pu_check(const slam_pf* h, double V, double G, double wheelbase, const double* Q, double dt, const double* z, int m,
             const double* R, double gate1, double gate2, PuArgs* a) {
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK(Q != nullptr, "null argument");
    ARG_CHECK(m >= 0 && m <= PU_MAX, "the proposal step with unknown correspondences takes at most 16 observations per call");
    ARG_CHECK(m == 0 || (z != nullptr && R != nullptr), "null argument");
    ARG_CHECK(std::isfinite(V) && std::isfinite(G) && std::isfinite(wheelbase) && std::isfinite(dt) && std::isfinite(gate1) &&
                  std::isfinite(gate2),
              "an argument is not finite");
    for (int i = 0; i < 4; ++i) ARG_CHECK(std::isfinite(Q[i]), "Q is not finite");
    for (int i = 0; i < 4; ++i) a->R[i] = 0.0;
    if (m) {
        for (int i = 0; i < 4; ++i) {
            ARG_CHECK(std::isfinite(R[i]), "R is not finite");
            a->R[i] = R[i];
        }
        for (int i = 0; i < 2 * m; ++i) ARG_CHECK(std::isfinite(z[i]), "an observation is not finite");
    }
    ARG_CHECK(Q[0] > 0.0, "Q is not positive definite");
    a->lq00 = sqrt(Q[0]);
    a->lq10 = 0.5 * (Q[1] + Q[2]) / a->lq00;
    ARG_CHECK(Q[3] - a->lq10 * a->lq10 > 0.0, "Q is not positive definite");
    a->lq11 = sqrt(Q[3] - a->lq10 * a->lq10);
    ARG_CHECK(h->n == h->n_global && h->d_peers == nullptr,
              "the proposal step with unknown correspondences needs the whole filter on this shard, without peers");
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_pf_proposal_limits(int out[4]) {
    ARG_CHECK(out != nullptr, "null argument");
    out[0] = PU_MAX; out[1] = 0; out[2] = 0; out[3] = 0;
    return SLAM_OK;
}

extern "C" int slam_pf_step_proposal_unknown(slam_pf_t h, double V, double G, double wheelbase, const double Q[4], double dt,
                                             const double* z, int m, const double R[4], double gate1, double gate2,
                                             int32_t* d_assoc, double out[3]) {
    SLAM_RANGE();
    PuArgs a;
    ARG_CHECK(out != nullptr, "null argument");
    int rc = pu_check(h, V, G, wheelbase, Q, dt, z, m, R, gate1, gate2, &a);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    if (m && (rc = pf_materialise(h))) return rc;             // the sweep reads every slot of buffer h->cur
    const double* dz = h->h_obs_dev;
    const int32_t* di = h->h_ids_dev;
    if (m && (rc = pf_stage(h, z, nullptr, m, &dz, &di))) return rc;
    const double pend = pf_take_pending(h);
    const int nl = m ? h->nl : 0;                             // no observation: the draw and the statistics only
#define PU_LAUNCH                                                                                                                  \
    hipLaunchKernelGGL(pf_proposal_unknown_kernel<T>, dim3(grid_for(h->n)), dim3(PU_WG), 0, h->stream, (T*)h->pose[h->pcur],       \
                       LmView<T>{h->d_lmtab}, h->cur, (T*)h->logw, h->n, h->first, h->step, h->seed, (T)V, (T)G, (T)wheelbase,     \
                       (T)a.lq00, (T)a.lq10, (T)a.lq11, (T)dt, nl, dz, m, (T)a.R[0], (T)a.R[1], (T)a.R[2], (T)a.R[3], (T)gate1,    \
                       (T)gate2, (T)pend, d_assoc, h->d_part)
    PF_DISPATCH(h, PU_LAUNCH, PU_LAUNCH);
#undef PU_LAUNCH
    HIP_TRY(hipGetLastError());
    if (m && (rc = pf_stage_done(h))) return rc;
    h->step += 1;
    double s[7];
    if ((rc = pf_fold_and_read(h, 1, s))) return rc;
    out[0] = s[0]; out[1] = s[1]; out[2] = s[2];
    return SLAM_OK;
}

extern "C" int slam_pf_associate_proposal(slam_pf_t h, double V, double G, double wheelbase, const double Q[4], double dt,
                                          const double* z, int m, const double R[4], double gate1, double gate2,
                                          int32_t* d_assoc, void* d_nis) {
    SLAM_RANGE();
    PuArgs a;
    int rc = pu_check(h, V, G, wheelbase, Q, dt, z, m, R, gate1, gate2, &a);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    if (m == 0 || (d_assoc == nullptr && d_nis == nullptr)) return SLAM_OK;
    if ((rc = pf_materialise(h))) return rc;
    const double* dz;
    const int32_t* di;
    if ((rc = pf_stage(h, z, nullptr, m, &dz, &di))) return rc;
#define PU_LAUNCH                                                                                                                  \
    hipLaunchKernelGGL(pf_associate_proposal_kernel<T>, dim3(grid_for(h->n)), dim3(PU_WG), 0, h->stream,                           \
                       (const T*)h->pose[h->pcur], LmView<T>{h->d_lmtab}, h->cur, h->n, (T)V, (T)G, (T)wheelbase, (T)a.lq00,       \
                       (T)a.lq10, (T)a.lq11, (T)dt, h->nl, dz, m, (T)a.R[0], (T)a.R[1], (T)a.R[2], (T)a.R[3], (T)gate1, (T)gate2,  \
                       d_assoc, (T*)d_nis)
    PF_DISPATCH(h, PU_LAUNCH, PU_LAUNCH);
#undef PU_LAUNCH
    HIP_TRY(hipGetLastError());
    return pf_stage_done(h);
}
