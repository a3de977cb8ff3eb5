// pf_evidence.hip -- landmark evidence of the unknown-correspondence particle filter (include/slamhip_evidence.h): one int8
// existence counter per (slot, particle), raised by a match, lowered when the landmark lies inside the sensor's field of view and
// was not observed; below zero the record is discarded (Probabilistic Robotics, Table 13.1).  libslamhip_evidence.so.
//
// One pass over the records of buffer `cur` (chunk by chunk through LmView) and the counters, bound by HBM: three of a record's
// five rows (x, y, Pxx) are read, one counter byte is read and -- where it changed -- written, a record is rewritten only on a
// prune: about 13 to 14 B per (slot, particle) in fp32, 25 to 26 B in fp64, against the 20 / 40 B the sweep of
// slam_pf_step_unknown reads.
//
//   grid (slabs of EV_SLAB particles, spans of `span` slots), 256 threads; a thread owns EV_PER particles
//   VEC    n a multiple of 4 and the decisions 16-byte aligned: the thread's particles are CONSECUTIVE, a row moves as one 16-byte
//          load (fp64: two), the four counters as one 4-byte word, the decisions as one int4 per observation
//   !VEC   any n: the thread's particles are 256 apart (every load of a wave is contiguous), counters move as bytes
//   The thread reads its particles' m decisions once and folds them into one 64-bit matched mask per particle:
//   bit (a & 63) where (a >> 6) == the span's group of 64 slots.  A negative decision has a negative group and never matches; a
//   decision beyond the map sets a bit no slot of the map tests.  Nothing is ever indexed with a decision.
//   `span` (a power of two, 16 .. 64, the host's choice) divides a group of 64 slots among several workgroups when the slabs alone
//   would leave compute units idle (262144 particles are 256 slabs); the decisions are then read once per span.
//   The slots of a span are taken kEvU at a time: all their loads are issued before the first is used.
//   The geometry runs only where it decides (in use, counter live, unmatched), the bearing only inside r_max.
//
// The four counts are integer sums: xor butterfly inside the wave, the four waves through LDS, one integer atomic per count and
// workgroup.  Integer addition: the totals do not depend on the order.
#include <cmath>

#include "pf_device.h"
#include "../../include/slamhip_evidence.h"

struct slam_pf_evidence {
    slam_pf* h;                      // borrowed
    int8_t* c[2];                    // [nl][n] counters, two buffers (the resampling gather is out of place)
    int cur;
    int32_t* d_dec;                  // [EV_MAXOBS][n] decisions of slam_pf_step_unknown_evidence
    unsigned long long* d_tot;       // [4] the counts of the last pass
};

namespace {

constexpr int EV_PER = 4;                    // particles per thread
constexpr int EV_WG = 256;
constexpr int EV_SLAB = EV_WG * EV_PER;      // particles per workgroup
constexpr int EV_GROUP = 64;                 // slots per matched mask
constexpr int EV_SPAN_MIN = 16;              // fewest slots a workgroup takes
constexpr int EV_WG_TARGET = 1024;           // workgroups from which the span is not divided further (four per compute unit)
constexpr int EV_MAXOBS = SLAM_PF_EVIDENCE_MAXOBS;
constexpr int EV_EMPTY = SLAM_PF_EVIDENCE_EMPTY;
constexpr int EV_GATHER_LMS = 16;            // slots per workgroup of the resampling gather

template <typename T>
constexpr int kEvU = sizeof(T) == 4 ? 4 : 2; // slots in flight per thread

// the thread's four values of one row: particles base, base + ST, ... (VEC: one 16-byte load, or two for fp64)
template <typename T, bool VEC>
__device__ __forceinline__ void ev_load4(const T* __restrict__ row, int64_t base, const bool (&ok)[EV_PER], T fill, T (&v)[EV_PER]) {
    if constexpr (VEC) {
        if (ok[0]) {                             // (n is a multiple of 4: the whole vector is inside)
            if constexpr (sizeof(T) == 4) {
                const float4 q = *reinterpret_cast<const float4*>(row + base);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                const double2 q0 = *reinterpret_cast<const double2*>(row + base), q1 = *reinterpret_cast<const double2*>(row + base + 2);
                v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < EV_PER; ++j) v[j] = fill;
        }
    } else {
#pragma unroll
        for (int j = 0; j < EV_PER; ++j) v[j] = ok[j] ? row[base + (int64_t)j * EV_WG] : fill;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(EV_WG) void pf_evidence_kernel(LmView<T> lv, int buf, const T* __restrict__ pose, int8_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ assoc, int64_t n, int nl, int m, int span,
                                                            T r_max, T half_fov, int inc, int dec, int init, int cap,
                                                            unsigned long long* __restrict__ totals) {
    constexpr int U = kEvU<T>;
    constexpr int64_t ST = VEC ? 1 : EV_WG;
    __shared__ unsigned s_tot[EV_WG / 64][4];
    const int64_t base = (int64_t)blockIdx.x * EV_SLAB + (VEC ? (int64_t)threadIdx.x * EV_PER : (int64_t)threadIdx.x);
    bool ok[EV_PER];
#pragma unroll
    for (int j = 0; j < EV_PER; ++j) ok[j] = base + (int64_t)j * ST < n;
    const int l_begin = (int)blockIdx.y * span;
    const int l_end = l_begin + span < nl ? l_begin + span : nl;
    const int group = l_begin / EV_GROUP;

    T px[EV_PER], py[EV_PER], pphi[EV_PER];
    ev_load4<T, VEC>(pose, base, ok, (T)0, px);
    ev_load4<T, VEC>(pose + n, base, ok, (T)0, py);
    ev_load4<T, VEC>(pose + 2 * n, base, ok, (T)0, pphi);

    // the matched mask of each of the thread's particles for this group of 64 slots
    unsigned long long mask[EV_PER] = {0ull, 0ull, 0ull, 0ull};
    for (int i = 0; i < m; ++i) {
        const int32_t* __restrict__ arow = assoc + (size_t)i * (size_t)n;
        int32_t a[EV_PER];
        if constexpr (VEC) {
            int4 q = make_int4(-1, -1, -1, -1);
            if (ok[0]) q = *reinterpret_cast<const int4*>(arow + base);
            a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < EV_PER; ++j) a[j] = ok[j] ? arow[base + (int64_t)j * EV_WG] : -1;
        }
#pragma unroll
        for (int j = 0; j < EV_PER; ++j)
            if ((a[j] >> 6) == group) mask[j] |= 1ull << (a[j] & 63);      // compared, never used as an index
    }

    unsigned n_use = 0, n_new = 0, n_dec = 0, n_cut = 0;
    for (int l0 = l_begin; l0 < l_end; l0 += U) {
        T lx[U][EV_PER], ly[U][EV_PER], pxx[U][EV_PER];
        int cv[U][EV_PER];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int l = l0 + u;
            if (l < l_end) {                         // uniform
                const T* __restrict__ rows = lv.rows(buf, l, n);
                ev_load4<T, VEC>(rows, base, ok, (T)0, lx[u]);
                ev_load4<T, VEC>(rows + n, base, ok, (T)0, ly[u]);
                ev_load4<T, VEC>(rows + 2 * n, base, ok, (T)-1, pxx[u]);
                const int8_t* __restrict__ crow = cnt + (size_t)l * (size_t)n;
                if constexpr (VEC) {
                    uint32_t w = 0x80808080u;
                    if (ok[0]) w = *reinterpret_cast<const uint32_t*>(crow + base);
#pragma unroll
                    for (int j = 0; j < EV_PER; ++j) cv[u][j] = (int)(int8_t)(w >> (8 * j));
                } else {
#pragma unroll
                    for (int j = 0; j < EV_PER; ++j) cv[u][j] = ok[j] ? (int)crow[base + (int64_t)j * EV_WG] : EV_EMPTY;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int l = l0 + u;
            if (l >= l_end) break;                   // uniform
            int cn[EV_PER];
            bool changed = false;
#pragma unroll
            for (int j = 0; j < EV_PER; ++j) {
                const int c = cv[u][j];
                cn[j] = c;
                if (!ok[j]) continue;
                const bool used = !(pxx[u][j] < (T)0);
                bool cut = false;
                if (!used) {
                    cn[j] = EV_EMPTY;                                                   // 1. a free slot
                } else if (c == EV_EMPTY) {
                    cn[j] = init;                                                       // 2. created since the last pass
                    ++n_new;
                } else if ((mask[j] >> (l & 63)) & 1ull) {
                    cn[j] = c + inc < cap ? c + inc : cap;                              // 3. matched
                } else {
                    const T dx = lx[u][j] - px[j], dy = ly[u][j] - py[j];
                    const T d = sqrt(dx * dx + dy * dy);
                    if (d <= r_max) {
                        const T b = wrap_pi<T>(atan2(dy, dx) - pphi[j]);
                        if (fabs(b) <= half_fov) {                                      // 4. in view and not observed
                            ++n_dec;
                            cn[j] = c - dec;
                            if (cn[j] < 0) {
                                cn[j] = EV_EMPTY;
                                cut = true;
                                ++n_cut;
                                T* __restrict__ rows = lv.rows(buf, l, n) + (base + (int64_t)j * ST);       // the empty record of pf_clear_lm_kernel
                                rows[0] = (T)0; rows[n] = (T)0; rows[2 * n] = (T)-1; rows[3 * n] = (T)0; rows[4 * n] = (T)0;
                            }
                        }
                    }
                }
                if (used && !cut) ++n_use;
                changed |= cn[j] != c;
            }
            int8_t* __restrict__ crow = cnt + (size_t)l * (size_t)n;
            if constexpr (VEC) {
                if (changed) {
                    uint32_t w = 0u;
#pragma unroll
                    for (int j = 0; j < EV_PER; ++j) w |= (uint32_t)(uint8_t)cn[j] << (8 * j);
                    *reinterpret_cast<uint32_t*>(crow + base) = w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < EV_PER; ++j)
                    if (ok[j] && cn[j] != cv[u][j]) crow[base + (int64_t)j * EV_WG] = (int8_t)cn[j];
            }
        }
    }

    unsigned t[4] = {n_use, n_new, n_dec, n_cut};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) t[i] += __shfl_xor(t[i], off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) s_tot[wave][i] = t[i];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned s = ((s_tot[0][threadIdx.x] + s_tot[1][threadIdx.x]) + s_tot[2][threadIdx.x]) + s_tot[3][threadIdx.x];
        if (s) atomicAdd(totals + threadIdx.x, (unsigned long long)s);
    }
}

// the counters follow their particles: dst[l][p] = src[l][anc[p]].  grid (ceil(n / 256), ceil(nl / EV_GATHER_LMS))
__global__ __launch_bounds__(256) void pf_evidence_gather_kernel(const int8_t* __restrict__ src, int8_t* __restrict__ dst,
                                                                 const int32_t* __restrict__ anc, int64_t n, int nl) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int64_t a = anc[p];
    if (a < 0 || a >= n) a = p;                      // (pf_ancestor_kernel writes 0 .. n - 1)
    const int l0 = (int)blockIdx.y * EV_GATHER_LMS;
    const int l1 = l0 + EV_GATHER_LMS < nl ? l0 + EV_GATHER_LMS : nl;
    for (int l = l0; l < l1; ++l) dst[(size_t)l * (size_t)n + p] = src[(size_t)l * (size_t)n + a];
}

int ev_live(const slam_pf_evidence* ev) {
    ARG_CHECK(ev != nullptr && ev->h != nullptr, "null evidence object");
    ARG_CHECK(ev->h->d_peers == nullptr && ev->h->n == ev->h->n_global,
              "landmark evidence supports only a filter that lives wholly on one shard, without peers");
    return SLAM_OK;
}

int ev_check(const slam_pf_evidence* ev, const int32_t* d_assoc, int m, double r_max, double half_fov, int inc, int dec, int init,
             int cap) {
    const int rc = ev_live(ev);
    if (rc) return rc;
    ARG_CHECK(m >= 0 && m <= EV_MAXOBS, "the evidence update takes the decisions of at most 64 observations");
    ARG_CHECK(m == 0 || d_assoc != nullptr, "null decisions");
    ARG_CHECK(std::isfinite(r_max) && r_max > 0.0, "r_max must be positive and finite");
    ARG_CHECK(half_fov > 0.0 && half_fov <= PF_PI, "half_fov must be in (0, pi]");
    ARG_CHECK(inc >= 1 && dec >= 1, "inc and dec must be at least 1");
    ARG_CHECK(init >= 0 && init <= cap && cap <= 127, "need 0 <= init <= cap <= 127");
    return SLAM_OK;
}

// the pass itself; the arguments have been checked
int ev_update(slam_pf_evidence* ev, const int32_t* d_assoc, int m, double r_max, double half_fov, int inc, int dec, int init, int cap,
              int64_t counts[4]) {
    slam_pf* h = ev->h;
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    int rc;
    if ((rc = pf_materialise(h))) return rc;                  // every record to (buffer cur, its particle's slot)
    if (inc > 256) inc = 256;                                 // (a live counter is at most 127: the same result, no overflow)
    if (dec > 256) dec = 256;
    const int64_t n = h->n;
    const int nl = h->nl;
    HIP_TRY(hipMemsetAsync(ev->d_tot, 0, 4 * sizeof(unsigned long long), h->stream));
    const int slabs = (int)((n + EV_SLAB - 1) / EV_SLAB);
    int span = EV_GROUP;
    while (span > EV_SPAN_MIN && (int64_t)slabs * ((nl + span - 1) / span) < EV_WG_TARGET) span >>= 1;
    const dim3 grid(slabs, (nl + span - 1) / span);
    const bool vec = n % 4 == 0 && (m == 0 || ((uintptr_t)d_assoc & 15) == 0);
#define EV_LAUNCH(VEC)                                                                                                              \
    hipLaunchKernelGGL((pf_evidence_kernel<T, VEC>), grid, dim3(EV_WG), 0, h->stream, LmView<T>{h->d_lmtab}, h->cur,                \
                       (const T*)h->pose[h->pcur], ev->c[ev->cur], d_assoc, n, nl, m, span, (T)r_max, (T)half_fov, inc, dec, init, cap, \
                       ev->d_tot)
    if (nl == 0 || n == 0) {
    } else if (vec) {
        PF_DISPATCH(h, EV_LAUNCH(true), EV_LAUNCH(true));
    } else {
        PF_DISPATCH(h, EV_LAUNCH(false), EV_LAUNCH(false));
    }
#undef EV_LAUNCH
    HIP_TRY(hipGetLastError());
    if (counts) {
        unsigned long long t[4];
        HIP_TRY(hipMemcpyAsync(t, ev->d_tot, sizeof(t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int i = 0; i < 4; ++i) counts[i] = (int64_t)t[i];
    }
    return SLAM_OK;
}

void ev_free(slam_pf_evidence* ev) {
    void* devs[] = {ev->c[0], ev->c[1], ev->d_dec, ev->d_tot};
    for (void* d : devs)
        if (d) (void)hipFree(d);
    delete ev;
}

}  // namespace

extern "C" int slam_pf_evidence_create(slam_pf_evidence_t* out, slam_pf_t h) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr && h != nullptr, "null argument");
    *out = nullptr;
    ARG_CHECK(h->n == h->n_global, "landmark evidence needs the whole filter on this shard (sharded filters are not supported)");
    ARG_CHECK(h->d_peers == nullptr, "landmark evidence does not support a filter with peers attached");
    HIP_TRY(hipSetDevice(h->device));
    slam_pf_evidence* ev = new slam_pf_evidence();
    ev->h = h;
    ev->c[0] = ev->c[1] = nullptr;
    ev->d_dec = nullptr;
    ev->d_tot = nullptr;
    ev->cur = 0;
    const size_t cbytes = (size_t)h->nl * (size_t)h->n;
    hipError_t e = hipSuccess;
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = hipMalloc((void**)&ev->c[b], cbytes ? cbytes : 16);
        if (e == hipSuccess) e = hipMemsetAsync(ev->c[b], 0x80, cbytes ? cbytes : 16, h->stream);       // EMPTY = -128
    }
    if (e == hipSuccess) e = hipMalloc((void**)&ev->d_dec, sizeof(int32_t) * (size_t)EV_MAXOBS * (size_t)h->n);
    if (e == hipSuccess) e = hipMalloc((void**)&ev->d_tot, 4 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        slam_set_error("slam_pf_evidence_create: %s", hipGetErrorString(e));
        ev_free(ev);
        return e == hipErrorOutOfMemory ? SLAM_E_NOMEM : SLAM_E_HIP;
    }
    *out = ev;
    return SLAM_OK;
}

extern "C" int slam_pf_evidence_destroy(slam_pf_evidence_t ev) {
    ARG_CHECK(ev != nullptr, "null evidence object");
    if (ev->h) {
        (void)hipSetDevice(ev->h->device);
        (void)hipStreamSynchronize(ev->h->stream);
    }
    ev_free(ev);
    return SLAM_OK;
}

extern "C" int slam_pf_evidence_update(slam_pf_evidence_t ev, const int32_t* d_assoc, int m, double r_max, double half_fov, int inc,
                                       int dec, int init, int cap, int64_t counts[4]) {
    SLAM_RANGE();
    const int rc = ev_check(ev, d_assoc, m, r_max, half_fov, inc, dec, init, cap);
    if (rc) return rc;
    return ev_update(ev, d_assoc, m, r_max, half_fov, inc, dec, init, cap, counts);
}

extern "C" int slam_pf_step_unknown_evidence(slam_pf_evidence_t ev, double V, double G, double wheelbase, const double Q[4], double dt,
                                             const double* z, int m, const double R[4], double gate1, double gate2, double r_max,
                                             double half_fov, int inc, int dec, int init, int cap, double out[3], int64_t counts[4]) {
    SLAM_RANGE();
    int rc = ev_check(ev, ev ? ev->d_dec : nullptr, m, r_max, half_fov, inc, dec, init, cap);
    if (rc) return rc;
    // (slam_pf_step_unknown checks its own arguments before it enqueues anything)
    if ((rc = slam_pf_step_unknown(ev->h, V, G, wheelbase, Q, dt, z, m, R, gate1, gate2, ev->d_dec, out))) return rc;
    return ev_update(ev, ev->d_dec, m, r_max, half_fov, inc, dec, init, cap, counts);
}

extern "C" int slam_pf_evidence_resample(slam_pf_evidence_t ev, double gmax, double u0) {
    SLAM_RANGE();
    int rc = ev_live(ev);
    if (rc) return rc;
    slam_pf* h = ev->h;
    if ((rc = slam_pf_resample_local(h, gmax, u0))) return rc;      // fills h->d_anc before its lazy and its eager branch
    const dim3 grid(grid_for(h->n), (h->nl + EV_GATHER_LMS - 1) / EV_GATHER_LMS);
    hipLaunchKernelGGL(pf_evidence_gather_kernel, grid, dim3(256), 0, h->stream, ev->c[ev->cur], ev->c[ev->cur ^ 1], h->d_anc, h->n,
                       h->nl);
    HIP_TRY(hipGetLastError());
    ev->cur ^= 1;
    return SLAM_OK;
}

extern "C" int slam_pf_evidence_get(slam_pf_evidence_t ev, int8_t* out) {
    const int rc = ev_live(ev);
    if (rc) return rc;
    ARG_CHECK(out != nullptr, "null argument");
    slam_pf* h = ev->h;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(out, ev->c[ev->cur], (size_t)h->nl * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}
