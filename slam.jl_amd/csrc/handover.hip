// handover.hip -- a state handed between the two filters on the device: slam_pf_to_ekf, slam_ekf_to_pf
// (include/slamhip_handover.h states both rules and the summation structure; tests/handover_ref.py runs them literally).
// libslamhip_handover.so.
//
// PARTICLES -> EKF.  P = Y'Y + blockdiag(0, sum what P_i,k) with Y[k][a] = sqrt(what_k) (z_ka - mu_a): a tall-skinny SYRK whose
// output tiles are the EKF's own (tile-major, block lower, edge E).
//   pass 1   slam_pf_map_sums (libslamhip.so): W, the means, the within-particle sums and the counts, fixed-order fp64.
//   ho_weights_kernel   sw_k = (T) sqrt(w_k / W) and the slabs' sums of w^2 (for Neff)
//   ho_gram_kernel      one workgroup of 256 threads per (tile (I, J), slab): rows of a dimension are contiguous over particles (the
//                       pose rows [3][n], the landmark rows through LmView of buffer cur after pf_materialise), so a chunk of HO_KC = 32
//                       particles of the 2 E dimensions is loaded coalesced along k, centred and scaled on the way into LDS
//                       ([dimension][HO_KC + 1]: the pad keeps the transposed fragment reads off one bank), and the four waves read their
//                       MFMA fragments from it transposed: wave (wr, wc) owns the quadrant (rows wr, columns wc) as 2 x 2 blocks of
//                       32 x 32 (fp32) / 16 x 16 (fp64).  The A operand takes the COLUMN dimensions, B the ROW dimensions, so a lane of
//                       the result holds one row of P and the partial's stores run along the tile's columns (column-major tiles).
//   ho_fold_kernel      sixteen workgroups per tile of dst below Tw: the slabs' partials in slab order in fp64, the within-particle term on
//                       the 2 x 2 diagonal blocks, +0.0 outside n', the store at p_off (p_store_sym inside a diagonal tile by r >= c).
// EKF -> PARTICLES.
//   ho_table_kernel     one workgroup, fp64: L_v = chol(P_vv), per landmark B_j, C_j and the not-positive-definite flag
//   ho_seed_kernel      grid (slabs of 1024 particles, groups of landmark slots): a thread draws its four particles' three normals,
//                       forms delta, and writes [lm][5][n] of its group (the group's table rows through LDS, read once per workgroup);
//                       group 0 also writes the poses and the log-weights.  VEC (n a multiple of 4): consecutive particles, 16-byte
//                       stores; otherwise the thread's particles are 256 apart.
#include <cmath>
#include <vector>

#include "pf_device.h"
#include "../../include/slamhip_handover.h"
#include "device_math.h"

namespace {

constexpr int HO_KC = 32;                  // particles per LDS chunk
constexpr int HO_WSLAB = 4096;             // particles per workgroup of ho_weights_kernel
constexpr uint32_t HO_STREAM = STREAM_HANDOVER;

// the MFMA tile (device_math.h) and SLAB: the particles of one partial
template <typename T> struct Ho : MfmaTile<T> {
    static constexpr int SLAB = sizeof(T) == 4 ? SLAM_HANDOVER_SLAB_F32 : SLAM_HANDOVER_SLAB_F64;
};

// ---- particles -> EKF ------------------------------------------------------------------------------------------------------

// sw[p] = (T) sqrt(w_p / W), w2[block] = the block's sum of w^2 (16 per thread, butterfly, the four waves in order)
template <typename T>
__global__ __launch_bounds__(256) void ho_weights_kernel(const T* __restrict__ logw, int64_t n, T pend, double W, T* __restrict__ sw,
                                                          double* __restrict__ w2) {
    __shared__ double sh[4];
    double a = 0.0;
    for (int j = 0; j < HO_WSLAB / 256; ++j) {
        const int64_t p = (int64_t)blockIdx.x * HO_WSLAB + (int64_t)j * 256 + threadIdx.x;
        if (p < n) {
            const double w = exp((double)(T)(logw[p] - pend));
            a += w * w;
            sw[p] = (T)sqrt(w / W);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) w2[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

template <typename T>
__global__ __launch_bounds__(256) void ho_x_kernel(T* __restrict__ x, const double* __restrict__ mu, int nn) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nn) x[i] = (T)mu[i];
}

// tile tq of the Tn (Tn + 1) / 2 tiles of the new state, band after band
__device__ __forceinline__ void ho_tile_of(int tq, int Tn, int* I, int* J) {
    int j = 0, base = 0;
    while (tq >= base + (Tn - j)) { base += Tn - j; ++j; }
    *J = j;
    *I = j + (tq - base);
}

template <typename T>
__global__ __launch_bounds__(256) void ho_gram_kernel(LmView<T> lv, int buf, const T* __restrict__ pose, const T* __restrict__ sw,
                                                       const double* __restrict__ mu, const int32_t* __restrict__ slots, int64_t n,
                                                       int nn, int Tn, int nslabs, T* __restrict__ part) {
    typedef Ho<T> H;
    constexpr int E = 1 << H::L, MB = H::MB;
    constexpr int LDK = HO_KC + 1;
    __shared__ T sY[2][E][LDK];                  // [0]: the row dimensions (tile row I), [1]: the column dimensions (tile row J)
    __shared__ const T* sRow[2][E];
    __shared__ double sMu[2][E];
    int I, J;
    ho_tile_of((int)blockIdx.x, Tn, &I, &J);
    const bool diag = I == J;
    // where each of the 2 E dimensions lives (null: beyond the state)
    for (int i = threadIdx.x; i < 2 * E; i += 256) {
        const int side = i >> H::L, dl = i & (E - 1);
        const int d = ((side ? J : I) << H::L) + dl;
        const T* r = nullptr;
        double m = 0.0;
        if (d < nn) {
            m = mu[d];
            r = d < 3 ? pose + (size_t)d * (size_t)n : lv.rows(buf, slots[(d - 3) >> 1], n) + (size_t)((d - 3) & 1) * (size_t)n;
        }
        sRow[side][dl] = r;
        sMu[side][dl] = m;
    }
    __syncthreads();
    const int64_t k_begin = (int64_t)blockIdx.y * H::SLAB;
    const int64_t k_end = k_begin + H::SLAB < n ? k_begin + H::SLAB : n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & (MB - 1), half = lane >> H::LSH;
    typename H::Acc acc[2][2];                   // [column block][row block]
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < H::NREG; ++r) acc[cb][rb][r] = (T)0;
    const int kl = threadIdx.x & (HO_KC - 1), r0 = threadIdx.x >> 5;      // the loads: particle k0 + kl of the rows r0, r0 + 8, ...
    // A chunk's values travel global -> registers -> LDS: ALL of the thread's loads of a chunk are issued at once, and the next
    // chunk's are issued before this chunk's MFMAs, so their latency runs under the matrix work (the first form issued four at a
    // time and waited for them inside the loop: DESIGN 5.10 has both timings).  A row beyond the state or a particle beyond the slab
    // loads nothing and holds 0: mu is 0 there, or the scale s is.
    constexpr int NI = 2 * E / 8;
    const int ni = diag ? NI / 2 : NI;           // (a diagonal tile has one set of dimensions)
    T v[NI], s;
    auto issue = [&](int64_t k0) {
        const int64_t k = k0 + kl;
        const bool kin = k < k_end;
        s = kin ? sw[k] : (T)0;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int i = r0 + 8 * j;
            const T* __restrict__ row = j < ni ? sRow[i >> H::L][i & (E - 1)] : nullptr;
            v[j] = (kin && row != nullptr) ? row[k] : (T)0;
        }
    };
    issue(k_begin);
    for (int64_t k0 = k_begin; k0 < k_end; k0 += HO_KC) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            if (j >= ni) break;                  // uniform
            const int i = r0 + 8 * j;
            const int side = i >> H::L, dl = i & (E - 1);
            double dv = (double)v[j] - sMu[side][dl];
            if (((side ? J : I) << H::L) + dl == 2) dv = mpi_to_pi_d(dv);
            sY[side][dl][kl] = (T)dv * s;
        }
        __syncthreads();
        if (k0 + HO_KC < k_end) issue(k0 + HO_KC);
        const int cs = diag ? 0 : 1;
#pragma unroll
        for (int kk = 0; kk < HO_KC / H::KS; ++kk) {
            const int kx = kk * H::KS + half;
            T a[2], b[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) a[cb] = sY[cs][2 * MB * wc + MB * cb + li][kx];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) b[rb] = sY[0][2 * MB * wr + MB * rb + li][kx];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[cb][rb] = H::mfma(a[cb], b[rb], acc[cb][rb]);
        }
        __syncthreads();
    }
    // the partial, in the tile's own order: entry (row, col) at col E + row
    T* __restrict__ out = part + ((size_t)blockIdx.x * (size_t)nslabs + (size_t)blockIdx.y) * (size_t)(E * E);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < H::NREG; ++r) {
                const int col = 2 * MB * wc + MB * cb + H::out_i(r, half);
                const int row = 2 * MB * wr + MB * rb + li;
                out[(size_t)col * E + row] = acc[cb][rb][r];
            }
}

// HO_FOLD_SEGS workgroups per tile (I, J), J <= I < Tw, of dst (a tile alone would leave most compute units idle: 45 tiles at C4)
constexpr int HO_FOLD_SEGS = 16;
template <typename T>
__global__ __launch_bounds__(256) void ho_fold_kernel(T* __restrict__ P, int ld, const T* __restrict__ part, const double* __restrict__ within,
                                                       int nn, int Tn, int nslabs) {
    typedef Ho<T> H;
    constexpr int E = 1 << H::L;
    const int I = blockIdx.x, J = blockIdx.y;
    if (J > I) return;
    const bool have = I < Tn;
    const size_t tq = (size_t)J * Tn - (size_t)J * (J - 1) / 2 + (size_t)(I - J);
    const T* __restrict__ src = part + tq * (size_t)nslabs * (size_t)(E * E);
    constexpr int SEG = E * E / HO_FOLD_SEGS;
    for (int e = (int)blockIdx.z * SEG + threadIdx.x; e < ((int)blockIdx.z + 1) * SEG; e += 256) {
        const int rl = e & (E - 1), cl = e >> H::L;
        const int r = (I << H::L) + rl, c = (J << H::L) + cl;
        if (I == J && r < c) continue;                                   // the mirror: written by the owner of (c, r)
        T v = (T)0;
        if (have && r < nn && c < nn) {
            double s = 0.0;
            for (int b = 0; b < nslabs; ++b) s += (double)src[(size_t)b * (size_t)(E * E) + e];
            if (c >= 3 && ((r - 3) >> 1) == ((c - 3) >> 1)) {            // (r >= c here or in a tile below the diagonal: r >= 3 too)
                const int l = (c - 3) >> 1;
                s += within[3 * (size_t)l + (r == c ? (((r - 3) & 1) ? 2 : 0) : 1)];
            }
            v = (T)s;
        }
        if (I == J) p_store_sym(P, ld, H::L, r, c, v);
        else P[p_off(ld, H::L, r, c)] = v;
    }
}

// the panel workspace's rows >= n must be zero for the down-date (ekf_api.hip does the same when an upload shrinks the map)
int ho_zero_panels(slam_ekf* h) {
    if (!h->kcap) return SLAM_OK;
    HIP_TRY(hipMemsetAsync(h->PHt, 0, sizeof(double) * (size_t)h->npad * h->kcap, h->stream));
    HIP_TRY(hipMemsetAsync(h->Kd, 0, sizeof(double) * (size_t)h->npad * h->kcap, h->stream));
    HIP_TRY(hipMemsetAsync(h->W1, 0, h->esz * (size_t)h->npad * 2 * h->kcap, h->stream));
    HIP_TRY(hipMemsetAsync(h->W2, 0, h->esz * (size_t)h->npad * 2 * h->kcap, h->stream));
    return SLAM_OK;
}

// the filter's grow-only read-out scratch (pf_map.hip keeps its partials there); the stream has been synchronised by the caller
int ho_workspace(slam_pf* h, size_t bytes) {
    if (bytes <= h->mapws_bytes) return SLAM_OK;
    if (h->d_mapws) (void)hipFree(h->d_mapws);
    h->d_mapws = nullptr;
    h->mapws_bytes = 0;
    bytes = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc(&h->d_mapws, bytes));
    h->mapws_bytes = bytes;
    return SLAM_OK;
}

int ho_check_pf(const slam_pf* pf) {
    ARG_CHECK(pf->n == pf->n_global && pf->d_peers == nullptr,
              "the hand-over supports only a filter that lives wholly on one shard, without peers");
    return SLAM_OK;
}

template <typename T>
int to_ekf_impl(slam_ekf* dst, slam_pf* src, const std::vector<int32_t>& slots, const std::vector<double>& sums, double info[4]) {
    typedef Ho<T> H;
    constexpr int E = 1 << H::L;
    const int cnt = (int)slots.size(), nn = 3 + 2 * cnt, n_old = 3 + 2 * dst->N;
    const int64_t n = src->n;
    const double W = sums[0];
    const int Td = dst->ld >> H::L, Tn = (nn + E - 1) >> H::L;
    int Tw = ((nn > n_old ? nn : n_old) + E - 1) >> H::L;
    if (Tw > Td) Tw = Td;
    const int nslabs = (int)((n + H::SLAB - 1) / H::SLAB), nwb = (int)((n + HO_WSLAB - 1) / HO_WSLAB);
    const size_t ntiles = (size_t)Tn * (Tn + 1) / 2;
    // the means and the within-particle term, from the sums of pass 1
    std::vector<double> host((size_t)nn + 3 * (size_t)cnt);
    host[0] = sums[1] / W; host[1] = sums[2] / W; host[2] = atan2(sums[6], sums[7]);
    for (int i = 0; i < cnt; ++i) {
        const double* r = &sums[(size_t)10 * (i + 1)];
        host[3 + 2 * (size_t)i] = r[1] / W; host[4 + 2 * (size_t)i] = r[2] / W;
        for (int k = 0; k < 3; ++k) host[(size_t)nn + 3 * (size_t)i + k] = r[6 + k] / W;
    }
    const size_t o_mu = 0, o_within = o_mu + slam_align256(sizeof(double) * nn), o_w2 = o_within + slam_align256(sizeof(double) * 3 * (cnt + 1)),
                 o_slots = o_w2 + slam_align256(sizeof(double) * nwb), o_sw = o_slots + slam_align256(sizeof(int32_t) * (cnt + 1)),
                 o_part = o_sw + slam_align256(sizeof(T) * (size_t)n), total = o_part + sizeof(T) * ntiles * (size_t)nslabs * (size_t)(E * E);
    int rc;
    HIP_TRY(hipStreamSynchronize(src->stream));                          // (the scratch may be replaced)
    if ((rc = ho_workspace(src, total))) return rc;
    char* ws = (char*)src->d_mapws;
    double* d_mu = (double*)(ws + o_mu);
    double* d_within = (double*)(ws + o_within);
    double* d_w2 = (double*)(ws + o_w2);
    int32_t* d_slots = (int32_t*)(ws + o_slots);
    T* d_sw = (T*)(ws + o_sw);
    T* d_part = (T*)(ws + o_part);
    std::vector<double> w2(nwb);
    const double pend = src->has_pending ? src->pending_shift : 0.0;     // read, not taken: src keeps its shift pending
    hipStream_t s = dst->stream;
    rc = slam_between(s, src->stream, [&]() -> int {
        int rcb;
        if (cnt < dst->N && (rcb = ho_zero_panels(dst))) return rcb;
        HIP_TRY(hipMemcpyAsync(d_mu, host.data(), sizeof(double) * nn, hipMemcpyHostToDevice, s));
        if (cnt) {
            HIP_TRY(hipMemcpyAsync(d_within, host.data() + nn, sizeof(double) * 3 * cnt, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), sizeof(int32_t) * cnt, hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(ho_weights_kernel<T>, dim3(nwb), dim3(256), 0, s, (const T*)src->logw, n, (T)pend, W, d_sw, d_w2);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ho_x_kernel<T>, dim3((nn + 255) / 256), dim3(256), 0, s, (T*)dst->x, (const double*)d_mu, nn);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ho_gram_kernel<T>, dim3((unsigned)ntiles, nslabs), dim3(256), 0, s, LmView<T>{src->d_lmtab}, src->cur,
                           (const T*)src->pose[src->pcur], (const T*)d_sw, (const double*)d_mu, (const int32_t*)d_slots, n, nn, Tn, nslabs,
                           d_part);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ho_fold_kernel<T>, dim3(Tw, Tw, HO_FOLD_SEGS), dim3(256), 0, s, (T*)dst->P, dst->ld, (const T*)d_part, (const double*)d_within,
                           nn, Tn, nslabs);
        HIP_TRY(hipGetLastError());
        // the launches have gone out: the host side follows the device at once
        dst->N = cnt;
        dst->grid_force = 1;                                             // the grid belongs to dst's old means
        dst->pmax_valid = 0;                                             // ... and the variance bound to its old matrix
        if ((rcb = launch_side_rebuild(dst))) return rcb;                // the packed 2 x 2 diagonal blocks follow the matrix
        HIP_TRY(hipMemcpyAsync(w2.data(), d_w2, sizeof(double) * nwb, hipMemcpyDeviceToHost, s));
        return SLAM_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (info) {
        double s2 = 0.0;
        for (int b = 0; b < nwb; ++b) s2 += w2[b];
        info[0] = W; info[1] = W * W / s2; info[2] = (double)n; info[3] = (double)cnt;
    }
    return SLAM_OK;
}

// ---- EKF -> particles ------------------------------------------------------------------------------------------------------
constexpr int HO_TAB_HEAD = 16;            // doubles: x_v[3], L_v[6] (00 10 11 20 21 22), then unused
constexpr int HO_TAB_ROW = 11;             // per landmark: m[2], B[2][3], Cxx, Cxy, Cyy
constexpr int HO_SEED_SLAB = 1024;         // particles per workgroup
constexpr int HO_SEED_LG = 16;             // landmark slots per workgroup

template <typename T>
__global__ __launch_bounds__(256) void ho_table_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld, const int32_t* __restrict__ ids,
                                                        int cnt, double* __restrict__ tab, int32_t* __restrict__ status) {
    constexpr int L = Ho<T>::L;
    __shared__ double sL[6];
    __shared__ int sBad;
    if (threadIdx.x == 0) {
        const double p00 = (double)P[p_off(ld, L, 0, 0)], p10 = (double)P[p_off(ld, L, 1, 0)], p11 = (double)P[p_off(ld, L, 1, 1)],
                     p20 = (double)P[p_off(ld, L, 2, 0)], p21 = (double)P[p_off(ld, L, 2, 1)], p22 = (double)P[p_off(ld, L, 2, 2)];
        int bad = 0;
        double l00 = 0, l10 = 0, l11 = 0, l20 = 0, l21 = 0, l22 = 0;
        if (!(p00 > 0.0)) bad = 1;
        if (!bad) {
            l00 = sqrt(p00); l10 = p10 / l00; l20 = p20 / l00;
            const double t = p11 - l10 * l10;
            if (!(t > 0.0)) bad = 1;
            else {
                l11 = sqrt(t); l21 = (p21 - l20 * l10) / l11;
                const double q = (p22 - l20 * l20) - l21 * l21;
                if (!(q > 0.0)) bad = 1;
                else l22 = sqrt(q);
            }
        }
        sL[0] = l00; sL[1] = l10; sL[2] = l11; sL[3] = l20; sL[4] = l21; sL[5] = l22;
        sBad = bad;
        for (int i = 0; i < 3; ++i) tab[i] = (double)x[i];
        for (int i = 0; i < 6; ++i) tab[3 + i] = sL[i];
        if (bad) status[0] = 1;
    }
    __syncthreads();
    if (sBad) return;
    const double l00 = sL[0], l10 = sL[1], l11 = sL[2], l20 = sL[3], l21 = sL[4], l22 = sL[5];
    for (int j = threadIdx.x; j < cnt; j += 256) {
        const int f = 3 + 2 * (ids[j] - 1);
        double* __restrict__ o = tab + HO_TAB_HEAD + (size_t)HO_TAB_ROW * j;
        double pv[2][3], B[2][3];
        for (int a = 0; a < 2; ++a) {
            for (int c = 0; c < 3; ++c) pv[a][c] = (double)P[p_off(ld, L, f + a, c)];
            // B_a P_vv = pv_a:  L y = pv_a', then L' b = y
            const double y0 = pv[a][0] / l00;
            const double y1 = (pv[a][1] - l10 * y0) / l11;
            const double y2 = ((pv[a][2] - l20 * y0) - l21 * y1) / l22;
            const double b2 = y2 / l22;
            const double b1 = (y1 - l21 * b2) / l11;
            const double b0 = ((y0 - l10 * b1) - l20 * b2) / l00;
            B[a][0] = b0; B[a][1] = b1; B[a][2] = b2;
        }
        const double pxx = (double)P[p_off(ld, L, f, f)], pxy = (double)P[p_off(ld, L, f + 1, f)], pyy = (double)P[p_off(ld, L, f + 1, f + 1)];
        const double cxx = pxx - ((B[0][0] * pv[0][0] + B[0][1] * pv[0][1]) + B[0][2] * pv[0][2]);
        const double cxy = pxy - ((B[1][0] * pv[0][0] + B[1][1] * pv[0][1]) + B[1][2] * pv[0][2]);
        const double cyy = pyy - ((B[1][0] * pv[1][0] + B[1][1] * pv[1][1]) + B[1][2] * pv[1][2]);
        if (!(cxx > 0.0) || !(cxx * cyy - cxy * cxy > 0.0)) status[0] = 1;
        o[0] = (double)x[f]; o[1] = (double)x[f + 1];
        for (int a = 0; a < 2; ++a)
            for (int c = 0; c < 3; ++c) o[2 + 3 * a + c] = B[a][c];
        o[8] = cxx; o[9] = cxy; o[10] = cyy;
    }
}

template <typename T>
__device__ __forceinline__ void ho_store4(T* __restrict__ row, int64_t base, const bool (&ok)[4], const T (&v)[4], bool vec) {
    if (vec) {
        if (ok[0]) {                             // (n is a multiple of 4: the whole vector is inside)
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<float4*>(row + base) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                *reinterpret_cast<double2*>(row + base) = make_double2(v[0], v[1]);
                *reinterpret_cast<double2*>(row + base + 2) = make_double2(v[2], v[3]);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ok[j]) row[base + (int64_t)j * 256] = v[j];
    }
}

// the first Box-Muller output of two words, as normals2 forms e1
template <typename T>
__device__ __forceinline__ T ho_normal1(uint32_t r0, uint32_t r1) {
    const T u1 = u01<T>(r0), u2 = u01<T>(r1);
    const T rad = m_sqrt<T>((T)-2.0 * m_log<T>(u1));
    if constexpr (kFast<T>) return rad * __builtin_amdgcn_cosf(u2);
    else return rad * cos((T)(2.0 * PF_PI) * u2);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void ho_seed_kernel(LmView<T> lv, int buf, T* __restrict__ pose, T* __restrict__ logw, int64_t n, int64_t first,
                                                       int nl, int cnt, uint32_t step, uint64_t seed, const double* __restrict__ tab, T lw) {
    __shared__ T sTab[HO_SEED_LG][HO_TAB_ROW];
    __shared__ T sHead[9];
    const int l0 = (int)blockIdx.y * HO_SEED_LG;
    const int l1 = l0 + HO_SEED_LG < nl ? l0 + HO_SEED_LG : nl;
    for (int i = threadIdx.x; i < HO_SEED_LG * HO_TAB_ROW; i += 256) {
        const int l = l0 + i / HO_TAB_ROW;
        sTab[i / HO_TAB_ROW][i % HO_TAB_ROW] = l < cnt ? (T)tab[HO_TAB_HEAD + (size_t)HO_TAB_ROW * l + i % HO_TAB_ROW] : (T)0;
    }
    if (threadIdx.x < 9) sHead[threadIdx.x] = (T)tab[threadIdx.x];
    __syncthreads();
    constexpr int64_t ST = VEC ? 1 : 256;
    const int64_t base = (int64_t)blockIdx.x * HO_SEED_SLAB + (VEC ? (int64_t)threadIdx.x * 4 : (int64_t)threadIdx.x);
    bool ok[4];
    T d0[4], d1[4], d2[4];
    const T L00 = sHead[3], L10 = sHead[4], L11 = sHead[5], L20 = sHead[6], L21 = sHead[7], L22 = sHead[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = base + (int64_t)j * ST;
        ok[j] = p < n;
        const uint64_t g = (uint64_t)(first + p);
        T e0, e1;
        normals2<T>(g, step, HO_STREAM, seed, e0, e1);
        uint32_t r[4];
        philox((uint32_t)g, (uint32_t)(g >> 32), step, HO_STREAM, (uint32_t)seed, (uint32_t)(seed >> 32), r);
        const T e2 = ho_normal1<T>(r[2], r[3]);
        d0[j] = L00 * e0;
        d1[j] = L10 * e0 + L11 * e1;
        d2[j] = (L20 * e0 + L21 * e1) + L22 * e2;
    }
    if (blockIdx.y == 0) {
        T v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sHead[0] + d0[j];
        ho_store4<T>(pose, base, ok, v, VEC);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sHead[1] + d1[j];
        ho_store4<T>(pose + n, base, ok, v, VEC);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = wrap_pi<T>(sHead[2] + d2[j]);
        ho_store4<T>(pose + 2 * n, base, ok, v, VEC);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = lw;
        ho_store4<T>(logw, base, ok, v, VEC);
    }
    for (int l = l0; l < l1; ++l) {
        const T* t = sTab[l - l0];
        T* __restrict__ rows = lv.rows(buf, l, n);
        T v[4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = l < cnt ? t[a] + ((t[2 + 3 * a] * d0[j] + t[3 + 3 * a] * d1[j]) + t[4 + 3 * a] * d2[j]) : (T)0;
            ho_store4<T>(rows + (size_t)a * (size_t)n, base, ok, v, VEC);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = t[8 + c];
            ho_store4<T>(rows + (size_t)(2 + c) * (size_t)n, base, ok, v, VEC);
        }
    }
}

template <typename T>
int to_pf_impl(slam_pf* dst, slam_ekf* src, const std::vector<int32_t>& ids) {
    const int cnt = (int)ids.size();
    const int64_t n = dst->n;
    const size_t o_tab = 0, o_ids = slam_align256(sizeof(double) * (HO_TAB_HEAD + (size_t)HO_TAB_ROW * (cnt + 1))),
                 o_status = o_ids + slam_align256(sizeof(int32_t) * (cnt + 1)), total = o_status + 256;
    int rc;
    HIP_TRY(hipStreamSynchronize(dst->stream));                          // (the scratch may be replaced)
    if ((rc = ho_workspace(dst, total))) return rc;
    char* ws = (char*)dst->d_mapws;
    double* d_tab = (double*)(ws + o_tab);
    int32_t* d_ids = (int32_t*)(ws + o_ids);
    int32_t* d_status = (int32_t*)(ws + o_status);
    hipStream_t s = dst->stream;
    int32_t status = 0;
    // the table, and its verdict, before anything of dst is written
    rc = slam_between(s, src->stream, [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
        if (cnt) HIP_TRY(hipMemcpyAsync(d_ids, ids.data(), sizeof(int32_t) * cnt, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ho_table_kernel<T>, dim3(1), dim3(256), 0, s, (const T*)src->x, (const T*)src->P, src->ld, (const int32_t*)d_ids, cnt,
                           d_tab, d_status);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&status, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return SLAM_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (status) {
        slam_set_error("slam_ekf_to_pf: the vehicle block or a landmark's conditional block is not positive definite");
        return SLAM_E_NOTPD;
    }
    // from here on dst is written: the bookkeeping of slam_pf_clear_landmarks and slam_pf_set_pose
    dst->has_pending = 0;
    dst->pending_shift = 0.0;
    const int B = dst->cur;
    const dim3 grid((unsigned)((n + HO_SEED_SLAB - 1) / HO_SEED_SLAB), (unsigned)((dst->nl + HO_SEED_LG - 1) / HO_SEED_LG));
    const T lw = (T)(-log((double)dst->n_global));
    if (n % 4 == 0)
        hipLaunchKernelGGL((ho_seed_kernel<T, true>), grid, dim3(256), 0, s, LmView<T>{dst->d_lmtab}, B, (T*)dst->pose[dst->pcur], (T*)dst->logw, n,
                           dst->first, dst->nl, cnt, dst->step, dst->seed, (const double*)d_tab, lw);
    else
        hipLaunchKernelGGL((ho_seed_kernel<T, false>), grid, dim3(256), 0, s, LmView<T>{dst->d_lmtab}, B, (T*)dst->pose[dst->pcur], (T*)dst->logw, n,
                           dst->first, dst->nl, cnt, dst->step, dst->seed, (const double*)d_tab, lw);
    HIP_TRY(hipGetLastError());
    for (int l = 0; l < dst->nl; ++l) {
        if (dst->ltab[l] >= 0) {                 // every slot of buffer cur was just overwritten: plain maps again
            dst->tref[dst->ltab[l]] -= 1;
            dst->ltab[l] = -1;
        }
        dst->lbuf[l] = (int8_t)B;
        dst->seen[l] = l < cnt ? 1 : 0;
    }
    dst->lazy_dirty = 0;
    dst->step += 1;
    HIP_TRY(hipStreamSynchronize(s));
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_pf_to_ekf(slam_ekf_t dst, slam_pf_t src, const int32_t* ids, int cnt, double info[4]) {
    SLAM_RANGE();
    ARG_CHECK(dst != nullptr && src != nullptr, "null handle");
    ARG_CHECK(dst->dtype == src->dtype, "the two states differ in dtype");
    ARG_CHECK(dst->device == src->device, "the two states live on different devices");
    int rc;
    if ((rc = ho_check_pf(src))) return rc;
    HIP_TRY(hipSetDevice(src->device));
    PF_LEGACY_ENTRY(src);                        // (the `seen` states come home; as slam_pf_download leaves the filter)
    std::vector<int32_t> slots;                  // 0-based
    if (ids == nullptr) {
        for (int l = 0; l < src->nl; ++l)
            if (src->seen[l]) slots.push_back(l);
    } else {
        ARG_CHECK(cnt >= 0, "cnt < 0");
        std::vector<char> taken((size_t)src->nl + 1, 0);
        for (int i = 0; i < cnt; ++i) {
            ARG_CHECK(ids[i] >= 1 && ids[i] <= src->nl, "landmark id out of range");
            ARG_CHECK(!taken[ids[i]], "duplicate landmark id");
            taken[ids[i]] = 1;
            slots.push_back(ids[i] - 1);
        }
    }
    cnt = (int)slots.size();
    if (cnt > dst->maxN) {
        slam_set_error("slam_pf_to_ekf: %d landmarks exceed capacity %d", cnt, dst->maxN);
        return SLAM_E_CAPACITY;
    }
    if (dst->pending_status && (rc = slam_ekf_sync(dst))) return rc;     // dst's deferred status; nothing written yet
    // pass 1: the fixed-order fp64 sums of the read-out (reads the records where they are, takes nothing, synchronises)
    std::vector<int32_t> ids1((size_t)cnt + 1, 1);
    for (int i = 0; i < cnt; ++i) ids1[i] = slots[i] + 1;
    std::vector<double> sums((size_t)10 * (cnt + 1));
    if ((rc = slam_pf_map_sums(src, ids1.data(), cnt, sums.data()))) return rc;
    const double W = sums[0];
    ARG_CHECK(std::isfinite(W) && W > 0.0, "the weights sum to zero or are not finite");
    for (int i = 0; i < cnt; ++i)
        if (sums[(size_t)10 * (i + 1) + 9] != (double)src->n) {
            slam_set_error("bad argument: landmark %d is in use in %.0f of %lld particles (the hand-over needs it in every particle)",
                           slots[i] + 1, sums[(size_t)10 * (i + 1) + 9], (long long)src->n);
            return SLAM_E_BADARG;
        }
    if ((rc = pf_materialise(src))) return rc;   // every record to (buffer cur, its particle's slot)
    return src->dtype == SLAM_F32 ? to_ekf_impl<float>(dst, src, slots, sums, info) : to_ekf_impl<double>(dst, src, slots, sums, info);
}

extern "C" int slam_ekf_to_pf(slam_pf_t dst, slam_ekf_t src, const int32_t* ids, int cnt) {
    SLAM_RANGE();
    ARG_CHECK(dst != nullptr && src != nullptr, "null handle");
    ARG_CHECK(dst->dtype == src->dtype, "the two states differ in dtype");
    ARG_CHECK(dst->device == src->device, "the two states live on different devices");
    int rc;
    if ((rc = ho_check_pf(dst))) return rc;
    std::vector<int32_t> list;                   // 1-based
    if (ids == nullptr) {
        for (int j = 1; j <= src->N; ++j) list.push_back(j);
    } else {
        ARG_CHECK(cnt >= 0, "cnt < 0");
        std::vector<char> taken((size_t)src->N + 1, 0);
        for (int i = 0; i < cnt; ++i) {
            ARG_CHECK(ids[i] >= 1 && ids[i] <= src->N, "landmark id out of range");
            ARG_CHECK(!taken[ids[i]], "duplicate landmark id");
            taken[ids[i]] = 1;
            list.push_back(ids[i]);
        }
    }
    if ((int)list.size() > dst->nl) {
        slam_set_error("slam_ekf_to_pf: %d landmarks exceed capacity %d", (int)list.size(), dst->nl);
        return SLAM_E_CAPACITY;
    }
    if (src->pending_status && (rc = slam_ekf_sync(src))) return rc;     // src's deferred status; dst untouched
    HIP_TRY(hipSetDevice(dst->device));
    PF_LEGACY_ENTRY(dst);
    return dst->dtype == SLAM_F32 ? to_pf_impl<float>(dst, src, list) : to_pf_impl<double>(dst, src, list);
}
