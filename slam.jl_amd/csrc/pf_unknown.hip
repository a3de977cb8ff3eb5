// pf_unknown.hip -- N4: the FastSLAM step with UNKNOWN correspondences as one sweep, up to 64 observations per call.
//
// slam_pf_step_unknown = slam_pf_predict + slam_pf_update_unknown + slam_pf_weight_stats in ONE kernel.  The legacy
// association kernel (pf_update_unknown_kernel, pf_legacy.hip) keeps the running minimum and its slot for each of its
// m <= 16 observations in one lane's registers; 64 observations do not fit a lane.  Here a workgroup holds 256 particles
// (the unit of the weight statistics: block_weight_stats and the fold must see the same 256-particle blocks as
// pf_stats_kernel for the three numbers to come out bit for bit) times G = ceil(m / 16) GROUPS of four waves; thread
// (g, t) owns observations 16 g .. 16 g + 15 of the workgroup's particle t.  (fp64: at most two groups, see kUnkGroups.)
//
//   predict   group 0 runs step_core's predict part (the code slam_pf_step shares with slam_pf_predict) and hands the new
//             pose to the other groups through LDS.
//   sweep     the slots are taken G at a time: group g reads slot l0 + g (every record is read from HBM once per
//             workgroup; the next round's record is requested before this round is scored), forms the quantities that do
//             not depend on the observation -- d, zp1, qa, qb, qc, logdet; d = -1 marks "no landmark here" (Pxx < 0) --
//             and passes them through LDS; then every group scores its 16 observations against the G slots in ascending
//             slot order.  The arithmetic per (slot, observation) is the legacy kernel's, term for term.  G == 1 skips the
//             LDS round trip: the same loop as the legacy kernel.
//   apply     all observations were associated against the map as it was before any update; the updates run in
//             OBSERVATION order: group 0's lanes apply theirs (lm_update / lm_init, the functions of the known-id sweep),
//             hand log-weight and the next unused slot to group 1's lanes through LDS, and so on.  A later group reads
//             records an earlier group's wave wrote: same workgroup, behind a barrier.
//   stats     block_weight_stats over the workgroup with only group 0's lanes valid: the other groups add exact zeros
//             behind the four waves' sums, so the partial record is the one pf_stats_kernel writes.
//
// Neither the 16 minima nor the decisions ever leave the registers (no scratch; see DESIGN, "unknown correspondences").
#include "pf_device.h"

namespace {

constexpr int UNK_GROUP = 16;                    // observations per lane
constexpr int UNK_GROUPS = 4;                    // groups of four waves per workgroup
constexpr int UNK_STEP_MAX = UNK_GROUP * UNK_GROUPS;
constexpr int UNK_WG = 256;                      // particles per workgroup

// what a slot contributes to every observation's score
template <typename T>
struct SlotQ {
    T d, zp1, qa, qb, qc, logdet;
};

template <typename T>
__device__ __forceinline__ SlotQ<T> slot_quantities(const LmRow<T>& r, T x, T y, T phi, T R00, T R10, T R01, T R11) {
    const T lx = r.lx, ly = r.ly, pxx = r.pxx, pxy = r.pxy, pyy = r.pyy;
    const T dx = lx - x, dy = ly - y;
    const T d2 = dx * dx + dy * dy;
    SlotQ<T> q;
    q.d = sqrt(d2);
    q.zp1 = atan2(dy, dx) - phi;
    const T d = q.d;
    const T h00 = dx / d, h01 = dy / d, h10 = -dy / d2, h11 = dx / d2;      // src/common.jl:162
    const T t00 = pxx * h00 + pxy * h01, t01 = pxx * h10 + pxy * h11;
    const T t10 = pxy * h00 + pyy * h01, t11 = pxy * h10 + pyy * h11;
    const T s00 = h00 * t00 + h01 * t10 + R00;                              // S = Hf Pf Hf' + R (:59), not symmetrised
    const T s01 = h00 * t01 + h01 * t11 + R01;
    const T s10 = h10 * t00 + h11 * t10 + R10;
    const T s11 = h10 * t01 + h11 * t11 + R11;
    const T det = s00 * s11 - s01 * s10;
    const T rdet = (T)1 / det;
    q.qa = s11 * rdet; q.qb = -(s01 + s10) * rdet; q.qc = s00 * rdet;
    q.logdet = log(det);
    return q;
}

// this lane's observations i0 .. i0 + 15 against slot l
template <typename T>
__device__ __forceinline__ void score_slot(const SlotQ<T>& q, int l, const double* s_obs, int i0, int m, T gate1, T gate2,
                                           T (&best_nd)[UNK_GROUP], int (&best_l)[UNK_GROUP], unsigned& near) {
#pragma unroll
    for (int i = 0; i < UNK_GROUP; ++i) {
        if (i0 + i < m) {
            const T v0 = (T)s_obs[2 * (i0 + i)] - q.d;
            const T v1 = wrap_pi<T>((T)s_obs[2 * (i0 + i) + 1] - q.zp1);          // :57
            const T nis = q.qa * v0 * v0 + q.qb * v0 * v1 + q.qc * v1 * v1;        // :60
            const T nd = nis + q.logdet;                                           // :61
            if (nis < gate1 && nd < best_nd[i]) { best_nd[i] = nd; best_l[i] = l; }     // strict: lowest slot wins a tie
            if (nis <= gate2) near |= 1u << i;
        }
    }
}

// NP: sweeps over the map a workgroup may make (lane (g, t) owns the 16-observation chunks g, g + ng, ...).  fp32 runs four
// groups and one sweep.  The fp64 score arithmetic (atan2, log, IEEE divisions beside 16 minima of two registers each) does
// not fit the 128 registers a 1024-thread workgroup leaves a lane, so fp64 runs at most two groups (512 threads, 256
// registers) and takes more than 32 observations in a second sweep; the first sweep's decisions wait in registers.
template <typename T>
constexpr int kUnkGroups = sizeof(T) == 4 ? UNK_GROUPS : 2;

template <typename T>
__global__ __launch_bounds__(UNK_WG * kUnkGroups<T>) void pf_step_unknown_kernel(
    T* __restrict__ pose, LmView<T> lv, int buf, T* __restrict__ logw, int64_t n, int64_t first, uint32_t step, uint64_t seed,
    T V, T G, T wheelbase, T sigV, T sigG, T dt, int nl, const double* __restrict__ z, int m, T R00, T R10, T R01, T R11,
    T gate1, T gate2, T pend, int32_t* __restrict__ assoc_out, double* __restrict__ part) {
    constexpr int NP = UNK_GROUPS / kUnkGroups<T>;
    // LDS: the observations (double, cast at use), the hand-over rows {x, y, phi, lw}[256] and next_free[256], then --
    // more than one group -- the slot quantities [ng][6][256]
    extern __shared__ double s_raw[];
    double* s_obs = s_raw;
    T* s_hand = reinterpret_cast<T*>(s_raw + 2 * UNK_STEP_MAX);
    int* s_free = reinterpret_cast<int*>(s_hand + 4 * UNK_WG);
    T* s_q = reinterpret_cast<T*>(s_free + UNK_WG);
    const int ng = (int)(blockDim.x >> 8);
    const int npass = ((m + UNK_GROUP - 1) / UNK_GROUP + ng - 1) / ng;
    const int t = threadIdx.x & (UNK_WG - 1), g = threadIdx.x >> 8;
    for (int i = threadIdx.x; i < 2 * m; i += blockDim.x) s_obs[i] = z[i];
    const int64_t pi = (int64_t)blockIdx.x * UNK_WG + t;
    const bool valid = pi < n;
    const int64_t p = valid ? pi : n - 1;          // idle lanes shadow the last particle, stores are masked
    T x = 0, y = 0, phi = 0, lw = 0;
    if (g == 0) {
        step_core<T, true>(pose, lv, nullptr, logw, n, first, step, seed, V, G, wheelbase, sigV, sigG, dt, (const T*)nullptr,
                           nullptr, nullptr, 0, R00, R10, R01, R11, pend, p, valid, x, y, phi, lw);
        if (ng > 1) { s_hand[t] = x; s_hand[UNK_WG + t] = y; s_hand[2 * UNK_WG + t] = phi; }
    }
    __syncthreads();
    if (g > 0) { x = s_hand[t]; y = s_hand[UNK_WG + t]; phi = s_hand[2 * UNK_WG + t]; }

    // ---- sweep: every observation against the map as it is now
    int dec[NP][UNK_GROUP];                        // slot >= 0 matched, -1 new, -2 dropped
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
        if (ps >= npass) break;                    // uniform
        const int i0 = (ps * ng + g) * UNK_GROUP;
        const T INF = (T)__builtin_inf();
        T best_nd[UNK_GROUP];
        int best_l[UNK_GROUP];
        unsigned near = 0u;
#pragma unroll
        for (int i = 0; i < UNK_GROUP; ++i) { best_nd[i] = INF; best_l[i] = -1; }
        if (ng == 1) {
            for (int l = 0; l < nl; ++l) {
                const T* row = lv.rows(buf, l, n) + p;
                if (row[2 * n] < (T)0) continue;
                const SlotQ<T> q = slot_quantities<T>(load_row<T>(row, n), x, y, phi, R00, R10, R01, R11);
                score_slot<T>(q, l, s_obs, i0, m, gate1, gate2, best_nd, best_l, near);
            }
        } else {
            const LmRow<T> none{0, 0, (T)-1, 0, 0};
            LmRow<T> nxt = none;
            if (g < nl) nxt = load_row<T>(lv.rows(buf, g, n) + p, n);
            for (int l0 = 0; l0 < nl; l0 += ng) {
                const LmRow<T> cur = nxt;
                nxt = none;
                if (l0 + ng + g < nl) nxt = load_row<T>(lv.rows(buf, l0 + ng + g, n) + p, n);
                SlotQ<T> q{(T)-1, 0, 0, 0, 0, 0};
                if (!(cur.pxx < (T)0)) q = slot_quantities<T>(cur, x, y, phi, R00, R10, R01, R11);
                T* mine = s_q + (size_t)g * 6 * UNK_WG + t;
                mine[0] = q.d; mine[UNK_WG] = q.zp1; mine[2 * UNK_WG] = q.qa; mine[3 * UNK_WG] = q.qb; mine[4 * UNK_WG] = q.qc;
                mine[5 * UNK_WG] = q.logdet;
                __syncthreads();
                for (int s = 0; s < ng && l0 + s < nl; ++s) {
                    const T* theirs = s_q + (size_t)s * 6 * UNK_WG + t;
                    SlotQ<T> o;
                    o.d = theirs[0];
                    if (o.d < (T)0) continue;
                    o.zp1 = theirs[UNK_WG]; o.qa = theirs[2 * UNK_WG]; o.qb = theirs[3 * UNK_WG]; o.qc = theirs[4 * UNK_WG];
                    o.logdet = theirs[5 * UNK_WG];
                    score_slot<T>(o, l0 + s, s_obs, i0, m, gate1, gate2, best_nd, best_l, near);
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int i = 0; i < UNK_GROUP; ++i) dec[ps][i] = best_l[i] >= 0 ? best_l[i] : (((near >> i) & 1u) ? -2 : -1);
    }

    // ---- apply, in observation order: chunk after chunk, i.e. group after group inside a sweep
    int next_free = 0;                                   // unused slots are handed out in ascending order
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
        if (ps >= npass) break;                          // uniform
        for (int gg = 0; gg < ng; ++gg) {
            if (g == gg) {
                const int i0 = (ps * ng + g) * UNK_GROUP;
                if (ng > 1 && (ps > 0 || gg > 0)) { lw = s_hand[3 * UNK_WG + t]; next_free = s_free[t]; }
#pragma unroll
                for (int i = 0; i < UNK_GROUP; ++i) {
                    if (i0 + i < m) {
                        const int a = dec[ps][i];
                        if (assoc_out && valid) assoc_out[(size_t)(i0 + i) * n + p] = a;
                        const T r = (T)s_obs[2 * (i0 + i)], b = (T)s_obs[2 * (i0 + i) + 1];
                        if (a >= 0) {
                            T* row = lv.rows(buf, a, n) + p;
                            const LmRow<T> cur = load_row<T>(row, n);
                            lm_update<T>(row, n, cur, x, y, phi, r, b, R00, R10, R01, R11, valid, lw);
                        } else if (a == -1) {
                            int slot = next_free;
                            while (slot < nl && !(lv.rows(buf, slot, n)[2 * n + p] < (T)0)) ++slot;
                            if (slot < nl) {
                                lm_init<T>(lv.rows(buf, slot, n) + p, n, x, y, phi, r, b, R00, R10, R01, R11, valid);
                                next_free = slot + 1;
                            }
                        }
                    }
                }
                if (ng > 1) { s_hand[3 * UNK_WG + t] = lw; s_free[t] = next_free; }
            }
            if (ng > 1) __syncthreads();                 // the next chunk's lanes read the records these ones wrote
        }
    }
    if (g == 0) {
        if (ng > 1) lw = s_hand[3 * UNK_WG + t];
        if (valid) logw[p] = lw;
    }
    block_weight_stats<T, false, false>(lw, x, y, phi, valid && g == 0, 1, part);
}

}  // namespace

/* predict + per-particle association + updates / new landmarks + local weight statistics as ONE sweep over the particles:
 * slam_pf_predict, slam_pf_update_unknown and slam_pf_weight_stats in one kernel, for m <= 64.  m <= 16: the same particles,
 * decisions and statistics bit for bit.  Synchronises (the caller needs Neff). */
extern "C" int slam_pf_step_unknown(slam_pf_t h, double V, double G, double wheelbase, const double Q[4], double dt,
                                    const double* z, int m, const double R[4], double gate1, double gate2, int32_t* d_assoc,
                                    double out[3]) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr && Q != nullptr && out != nullptr, "null argument");
    ARG_CHECK(m >= 0 && m <= UNK_STEP_MAX, "slam_pf_step_unknown takes at most 64 observations per call");
    ARG_CHECK(m == 0 || (z != nullptr && R != nullptr), "null argument");
    double Rz[4] = {0, 0, 0, 0};
    if (m) for (int i = 0; i < 4; ++i) Rz[i] = R[i];
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    int rc;
    if (m && (rc = pf_materialise(h))) return rc;             // the sweep reads every slot of buffer h->cur (collective with peers)
    const double* dz = h->h_obs_dev;
    const int32_t* di = h->h_ids_dev;
    if (m && (rc = pf_stage(h, z, nullptr, m, &dz, &di))) return rc;
    const double sV = sqrt(Q[0]), sG = sqrt(Q[3]);
    const double pend = pf_take_pending(h);
    const int chunks = m ? (m + UNK_GROUP - 1) / UNK_GROUP : 1;
    const int gmax = h->dtype == SLAM_F32 ? kUnkGroups<float> : kUnkGroups<double>;
    const int ng = chunks < gmax ? chunks : gmax;          // (fp64 beyond 32 observations: a second sweep, see the kernel)
    const int nl = m ? h->nl : 0;                             // no observation: predict and statistics only
    const size_t lds = sizeof(double) * 2 * UNK_STEP_MAX + h->esz * 4 * UNK_WG + sizeof(int) * UNK_WG +
                       (ng > 1 ? h->esz * 6 * UNK_WG * (size_t)ng : 0);
    PF_DISPATCH(h,
                hipLaunchKernelGGL(pf_step_unknown_kernel<T>, dim3(grid_for(h->n)), dim3(UNK_WG * ng), lds, h->stream,
                                   (T*)h->pose[h->pcur], LmView<T>{h->d_lmtab}, h->cur, (T*)h->logw, h->n, h->first, h->step, h->seed,
                                   (T)V, (T)G, (T)wheelbase, (T)sV, (T)sG, (T)dt, nl, dz, m, (T)Rz[0], (T)Rz[1], (T)Rz[2], (T)Rz[3],
                                   (T)gate1, (T)gate2, (T)pend, d_assoc, h->d_part),
                hipLaunchKernelGGL(pf_step_unknown_kernel<T>, dim3(grid_for(h->n)), dim3(UNK_WG * ng), lds, h->stream,
                                   (T*)h->pose[h->pcur], LmView<T>{h->d_lmtab}, h->cur, (T*)h->logw, h->n, h->first, h->step, h->seed,
                                   (T)V, (T)G, (T)wheelbase, (T)sV, (T)sG, (T)dt, nl, dz, m, (T)Rz[0], (T)Rz[1], (T)Rz[2], (T)Rz[3],
                                   (T)gate1, (T)gate2, (T)pend, d_assoc, h->d_part));
    HIP_TRY(hipGetLastError());
    if (m && (rc = pf_stage_done(h))) return rc;
    h->step += 1;
    double s[7];
    if ((rc = pf_fold_and_read(h, 1, s))) return rc;
    out[0] = s[0]; out[1] = s[1]; out[2] = s[2];
    return SLAM_OK;
}
