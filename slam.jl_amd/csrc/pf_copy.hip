// pf_copy.hip -- a FastSLAM particle set moved on the device: slam_pf_upload, slam_pf_copy, slam_pf_select, slam_pf_resize,
// slam_pf_get_meta, slam_pf_set_rng, slam_pf_pose_bins (include/slamhip_pfcopy.h states every rule; DESIGN 5.3d;
// tests/pfcopy_ref.py runs them literally).  libslamhip_pfcopy.so.
//
//     dst(k, q) = src(slot_k, anc_q)        anc = the identity (copy, select) or the ancestor table of a resampling of src's n
//                                           particles into dst's m slots (resize)
// No arithmetic on the records: a data-movement problem between two filters whose records lie in chunks of whole landmarks
// ([landmark][5][n], PfLmTab) with chunk shifts that may differ, and whose SOURCE records lie where lazy resampling left them:
// landmark l's record of particle p in buffer lbuf[l] at slot tab[ltab[l]][p].  src is read in place and never materialised.
//   pc_gather_kernel<T, ANC, VEC>   grid (slabs of 1024 dst particles, groups of PC_LG dst landmarks).  A thread owns four dst
//                       particles, loads their ancestors once (ANC) and a table's four entries once per run of landmarks behind
//                       that table, then moves five rows per landmark: all loads of a landmark are issued before its stores.  The
//                       per-landmark work list {source slot | fill code, table + 1 | buffer << 8} is indexed by blockIdx.y and
//                       the loop counter only (wave-uniform: scalar loads).  VEC (m a multiple of 4): consecutive particles, every
//                       row of both sides 16-byte aligned, 16-byte stores, and 16-byte loads where !ANC and the landmark has no
//                       table; otherwise the thread's particles are 256 apart and every access is one element.  Group 0 also moves
//                       the poses and the log-weights.  Values move as integers: bit for bit.  Stores are non-temporal (dst is read
//                       next by a sweep over all of it, far larger than the caches where the time matters).
//   pc_scan1 / pc_scan2 / pc_ancestor_kernel   the cdf of slam_pf_resample_local (block_scan1024, serial block offsets) and the
//                       binary search with the target formed with m.
//   pc_bins_kernel      the pose histogram's occupied cells: open addressing, compare-and-swap insert.
// OWNERSHIP: every element of dst's buffer cur, pose buffer and log-weights has exactly one writing thread (particle p < m:
// thread of slab p / 1024, landmark group l / PC_LG); src is only read.  No LDS in the gather, no private scratch beyond registers.
#include <cmath>
#include <vector>

#include "pf_device.h"
#include "../../include/slamhip_pfcopy.h"

namespace {

constexpr int PC_SLAB = 1024;              // dst particles per workgroup (256 threads x 4)
constexpr int PC_LG = 16;                  // dst landmarks per workgroup
constexpr int32_t PC_FILL0 = -1;           // work list: the all-zero record
constexpr int32_t PC_FILL1 = -2;           // work list: the unused record (0, 0, -1, 0, 0)

struct PcWork {
    int32_t slot;                // source landmark (0-based), or PC_FILL0 / PC_FILL1
    int32_t meta;                // (table + 1) | source buffer << 8
};

typedef unsigned vec4u __attribute__((ext_vector_type(4)));
typedef unsigned long long vec2ul __attribute__((ext_vector_type(2)));

template <typename T> struct Bits;
template <> struct Bits<float> { typedef uint32_t U; };
template <> struct Bits<double> { typedef uint64_t U; };

// four values of one row: base = the thread's first particle, stride 1 (VEC: one or two 16-byte pieces) or 256
template <typename U, bool VEC>
__device__ __forceinline__ void pc_load4(const U* __restrict__ row, int64_t base, const bool (&ok)[4], U (&v)[4]) {
    if constexpr (VEC) {
        if constexpr (sizeof(U) == 4) {
            const vec4u t = *reinterpret_cast<const vec4u*>(row + base);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            const vec2ul t0 = *reinterpret_cast<const vec2ul*>(row + base), t1 = *reinterpret_cast<const vec2ul*>(row + base + 2);
            v[0] = t0.x; v[1] = t0.y; v[2] = t1.x; v[3] = t1.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ok[j] ? row[base + (int64_t)j * 256] : (U)0;
    }
}

template <typename U>
__device__ __forceinline__ void pc_gather4(const U* __restrict__ row, const int64_t (&s)[4], U (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = row[s[j]];            // (s of a particle beyond m is 0: a valid slot, the value is not stored)
}

template <typename U, bool VEC>
__device__ __forceinline__ void pc_store4(U* __restrict__ row, int64_t base, const bool (&ok)[4], const U (&v)[4]) {
    if constexpr (VEC) {                         // (m is a multiple of 4 and ok[0] holds: the whole vector is inside)
        if constexpr (sizeof(U) == 4) {
            __builtin_nontemporal_store(vec4u{v[0], v[1], v[2], v[3]}, reinterpret_cast<vec4u*>(row + base));
        } else {
            __builtin_nontemporal_store(vec2ul{v[0], v[1]}, reinterpret_cast<vec2ul*>(row + base));
            __builtin_nontemporal_store(vec2ul{v[2], v[3]}, reinterpret_cast<vec2ul*>(row + base + 2));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ok[j]) __builtin_nontemporal_store(v[j], row + base + (int64_t)j * 256);
    }
}

template <typename T>
__device__ __forceinline__ typename Bits<T>::U pc_bits(T v) {
    typename Bits<T>::U u;
    __builtin_memcpy(&u, &v, sizeof(u));
    return u;
}

// n: particles of src, m: particles of dst (ANC == false: m == n).  lw: the uniform log-weight of a resize.
template <typename T, bool ANC, bool VEC>
__global__ __launch_bounds__(256) void pc_gather_kernel(LmView<T> dv, int dbuf, LmView<T> sv, const PcWork* __restrict__ work,
                                                         const int32_t* __restrict__ stabs, const int32_t* __restrict__ anc, int64_t n,
                                                         int64_t m, int nl, const T* __restrict__ spose, T* __restrict__ dpose,
                                                         const T* __restrict__ slogw, T* __restrict__ dlogw, T pend, int has_pend, T lw) {
    typedef typename Bits<T>::U U;
    constexpr int64_t ST = VEC ? 1 : 256;
    const int64_t base = (int64_t)blockIdx.x * PC_SLAB + (VEC ? (int64_t)threadIdx.x * 4 : (int64_t)threadIdx.x);
    if (base >= m) return;                       // (the thread's first particle is its lowest; no barrier below)
    bool ok[4];
    int64_t a[4], s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = base + (int64_t)j * ST;
        ok[j] = p < m;
        a[j] = !ok[j] ? 0 : (ANC ? (int64_t)anc[p] : p);
        s[j] = a[j];
    }
    if (blockIdx.y == 0) {
        U v[3][4];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const U* __restrict__ row = reinterpret_cast<const U*>(spose) + (size_t)r * (size_t)n;
            if constexpr (!ANC) pc_load4<U, VEC>(row, base, ok, v[r]);
            else pc_gather4<U>(row, a, v[r]);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) pc_store4<U, VEC>(reinterpret_cast<U*>(dpose) + (size_t)r * (size_t)m, base, ok, v[r]);
        U w[4];
        if constexpr (ANC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = pc_bits<T>(lw);
        } else {
            pc_load4<U, VEC>(reinterpret_cast<const U*>(slogw), base, ok, w);
            if (has_pend) {                      // what pf_shift_kernel would store
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    T x;
                    __builtin_memcpy(&x, &w[j], sizeof(x));
                    x -= pend;
                    w[j] = pc_bits<T>(x);
                }
            }
        }
        pc_store4<U, VEC>(reinterpret_cast<U*>(dlogw), base, ok, w);
    }
    const int l0 = (int)blockIdx.y * PC_LG;
    const int l1 = l0 + PC_LG < nl ? l0 + PC_LG : nl;
    int tprev = 0;                               // s = the slots behind table tprev - 1 (0: the ancestors themselves)
    for (int l = l0; l < l1; ++l) {
        const PcWork w = work[l];                // (uniform)
        U* __restrict__ drow = reinterpret_cast<U*>(dv.rows(dbuf, l, m));
        U v[5][4];
        if (w.slot < 0) {
            const U third = w.slot == PC_FILL1 ? pc_bits<T>((T)-1) : (U)0;
#pragma unroll
            for (int c = 0; c < 5; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[c][j] = c == 2 ? third : (U)0;
        } else {
            const int t = w.meta & 0xff;
            const U* __restrict__ srow = reinterpret_cast<const U*>(sv.rows((w.meta >> 8) & 1, w.slot, n));
            if (t != tprev) {
                const int32_t* __restrict__ tab = stabs + (size_t)(t ? t - 1 : 0) * (size_t)n;
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = t ? (int64_t)tab[a[j]] : a[j];
                tprev = t;
            }
            if (!ANC && t == 0) {
#pragma unroll
                for (int c = 0; c < 5; ++c) pc_load4<U, VEC>(srow + (size_t)c * (size_t)n, base, ok, v[c]);
            } else {
#pragma unroll
                for (int c = 0; c < 5; ++c) pc_gather4<U>(srow + (size_t)c * (size_t)n, s, v[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) pc_store4<U, VEC>(drow + (size_t)c * (size_t)m, base, ok, v[c]);
    }
}

// ---- the cdf and the ancestors of a resize: slam_pf_resample_local's, the target with m ----------------------------------------
template <typename T>
__global__ __launch_bounds__(SCAN_BLOCK) void pc_scan1_kernel(const T* __restrict__ logw, int64_t n, double gmax, double* __restrict__ cdf,
                                                               double* __restrict__ bsum, T pend) {
    __shared__ double sh16[16];
    const int64_t i = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const double c = block_scan1024(i < n ? exp((double)(T)(logw[i] - pend) - gmax) : 0.0, sh16);
    if (i < n) cdf[i] = c;
    if (threadIdx.x == SCAN_BLOCK - 1) bsum[blockIdx.x] = c;
}

// exclusive scan of the block totals in place; bsum[nb] = the total.  The additions run in index order on ONE thread (the order
// of pf_scan2_kernel: the table must be the exact one), out of LDS: the whole workgroup loads and stores.
constexpr int PC_SCAN2_CHUNK = 4096;
__global__ __launch_bounds__(256) void pc_scan2_kernel(double* __restrict__ bsum, int nb) {
    __shared__ double sh[PC_SCAN2_CHUNK];
    __shared__ double carry;
    if (threadIdx.x == 0) carry = 0.0;
    for (int base = 0; base < nb; base += PC_SCAN2_CHUNK) {
        const int cnt = nb - base < PC_SCAN2_CHUNK ? nb - base : PC_SCAN2_CHUNK;
        for (int i = threadIdx.x; i < cnt; i += 256) sh[i] = bsum[base + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            double run = carry;
            for (int i = 0; i < cnt; ++i) {
                const double v = sh[i];
                sh[i] = run;
                run += v;
            }
            carry = run;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < cnt; i += 256) bsum[base + i] = sh[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(256) void pc_ancestor_kernel(const double* __restrict__ cdf, const double* __restrict__ bsum, int nb, int64_t n,
                                                           int64_t m, double u0, int32_t* __restrict__ anc) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    const double total = bsum[nb];
    const double target = ((double)q + u0) / (double)m * total;
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const double c = cdf[mid] + bsum[mid / SCAN_BLOCK];
        if (c >= target) hi = mid; else lo = mid + 1;
    }
    anc[q] = (int32_t)lo;
}

// ---- the pose histogram -------------------------------------------------------------------------------------------------------
constexpr unsigned long long PC_EMPTY = ~0ull;

// out[0]: distinct keys, out[1]: != 0: a pose out of range or not finite
template <typename T>
__global__ __launch_bounds__(256) void pc_bins_kernel(const T* __restrict__ pose, int64_t n, double cell_xy, double cell_phi, long long ip_max,
                                                       unsigned long long* __restrict__ set, int log2_slots,
                                                       unsigned long long* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double x = (double)pose[p], y = (double)pose[n + p], phi = (double)pose[2 * n + p];
    const double fx = floor(x / cell_xy), fy = floor(y / cell_xy);
    double fp = floor((phi + PF_PI) / cell_phi);
    const double lim = 1048576.0;
    // (written so that a NaN fails every test)
    if (!(fx > -lim && fx < lim && fy > -lim && fy < lim) || !(phi - phi == 0.0)) {
        out[1] = 1ull;
        return;
    }
    if (fp < 0.0) fp = 0.0;
    if (fp > (double)ip_max) fp = (double)ip_max;
    const unsigned long long key = ((unsigned long long)((long long)fx + 1048576ll) << 42) |
                                   ((unsigned long long)((long long)fy + 1048576ll) << 21) | (unsigned long long)(long long)fp;
    const unsigned long long mask = (1ull << log2_slots) - 1ull;
    unsigned long long i = (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots);
    for (unsigned long long probe = 0; probe <= mask; ++probe, i = (i + 1) & mask) {     // (at most half of the slots fill up)
        unsigned long long seen = set[i];
        if (seen == PC_EMPTY) seen = atomicCAS(&set[i], PC_EMPTY, key);
        if (seen == PC_EMPTY) {                  // this thread put the key in
            atomicAdd(&out[0], 1ull);
            return;
        }
        if (seen == key) return;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the filter's grow-only read-out scratch (pf_map.hip keeps its partials there); the stream has been synchronised by the caller
int pc_workspace(slam_pf* h, size_t bytes) {
    if (bytes <= h->mapws_bytes) return SLAM_OK;
    if (h->d_mapws) (void)hipFree(h->d_mapws);
    h->d_mapws = nullptr;
    h->mapws_bytes = 0;
    bytes = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc(&h->d_mapws, bytes));
    h->mapws_bytes = bytes;
    return SLAM_OK;
}

int pc_check_pair(const slam_pf* dst, const slam_pf* src) {
    ARG_CHECK(dst != nullptr && src != nullptr, "null handle");
    ARG_CHECK(dst != src, "dst and src are the same handle");
    ARG_CHECK(dst->dtype == src->dtype, "the two filters differ in dtype");
    ARG_CHECK(dst->device == src->device, "the two filters live on different devices");
    ARG_CHECK(dst->n == dst->n_global && dst->first == 0 && dst->d_peers == nullptr && src->n == src->n_global && src->first == 0 &&
                  src->d_peers == nullptr,
              "both filters must live wholly on one shard, without peers");
    return SLAM_OK;
}

template <typename T, bool ANC>
int pc_launch_gather(slam_pf* dst, slam_pf* src, const PcWork* d_work, const int32_t* d_anc, T pend, int has_pend, T lw, hipStream_t s) {
    const int64_t n = src->n, m = dst->n;
    const dim3 grid((unsigned)((m + PC_SLAB - 1) / PC_SLAB), (unsigned)((dst->nl + PC_LG - 1) / PC_LG));
    // VEC needs every row of BOTH sides 16-byte aligned where 16-byte loads can happen (!ANC: n == m) and of dst always
    if (m % 4 == 0)
        hipLaunchKernelGGL((pc_gather_kernel<T, ANC, true>), grid, dim3(256), 0, s, LmView<T>{dst->d_lmtab}, dst->cur, LmView<T>{src->d_lmtab},
                           d_work, (const int32_t*)src->d_tab[src->tside], d_anc, n, m, dst->nl, (const T*)src->pose[src->pcur],
                           (T*)dst->pose[dst->pcur], (const T*)src->logw, (T*)dst->logw, pend, has_pend, lw);
    else
        hipLaunchKernelGGL((pc_gather_kernel<T, ANC, false>), grid, dim3(256), 0, s, LmView<T>{dst->d_lmtab}, dst->cur, LmView<T>{src->d_lmtab},
                           d_work, (const int32_t*)src->d_tab[src->tside], d_anc, n, m, dst->nl, (const T*)src->pose[src->pcur],
                           (T*)dst->pose[dst->pcur], (const T*)src->logw, (T*)dst->logw, pend, has_pend, lw);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// slots: the source landmark (0-based) of dst's landmarks 0 .. cnt.  Arguments are checked; both filters are in legacy mode.
template <typename T>
int pc_move(slam_pf* dst, slam_pf* src, const std::vector<int32_t>& slots, int fill, bool resize, double gmax, double u0, int32_t* anc_out) {
    const int cnt = (int)slots.size();
    const int64_t n = src->n, m = dst->n;
    const int nb = (int)((n + SCAN_BLOCK - 1) / SCAN_BLOCK);
    std::vector<PcWork> work((size_t)dst->nl);
    for (int k = 0; k < dst->nl; ++k) {
        if (k < cnt) {
            const int l = slots[k];
            work[k].slot = l;
            work[k].meta = (src->ltab[l] + 1) | (src->lbuf[l] ? 1 << 8 : 0);
        } else {
            work[k].slot = fill ? PC_FILL1 : PC_FILL0;
            work[k].meta = 0;
        }
    }
    const size_t o_work = 0, o_anc = o_work + slam_align256(sizeof(PcWork) * (size_t)dst->nl),
                 o_cdf = o_anc + slam_align256(resize ? sizeof(int32_t) * (size_t)m : 0), o_bsum = o_cdf + slam_align256(resize ? sizeof(double) * (size_t)n : 0),
                 total_bytes = o_bsum + slam_align256(resize ? sizeof(double) * ((size_t)nb + 1) : 0);
    int rc;
    HIP_TRY(hipStreamSynchronize(dst->stream));                          // (the scratch may be replaced)
    if ((rc = pc_workspace(dst, total_bytes))) return rc;
    char* ws = (char*)dst->d_mapws;
    PcWork* d_work = (PcWork*)(ws + o_work);
    int32_t* d_anc = (int32_t*)(ws + o_anc);
    double* d_cdf = (double*)(ws + o_cdf);
    double* d_bsum = (double*)(ws + o_bsum);
    const double pend = src->has_pending ? src->pending_shift : 0.0;     // read, not taken: src keeps its shift pending
    hipStream_t s = dst->stream;
    if (resize) {
        // the cdf and its total, read back before anything of dst is written
        double total = 0.0;
        rc = slam_between(s, src->stream, [&]() -> int {
            hipLaunchKernelGGL(pc_scan1_kernel<T>, dim3(nb), dim3(SCAN_BLOCK), 0, s, (const T*)src->logw, n, gmax, d_cdf, d_bsum, (T)pend);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(pc_scan2_kernel, dim3(1), dim3(256), 0, s, d_bsum, nb);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&total, d_bsum + nb, sizeof(double), hipMemcpyDeviceToHost, s));
            return SLAM_OK;
        });
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        ARG_CHECK(std::isfinite(total) && total > 0.0, "the weights sum to zero or are not finite");
    }
    // from here on dst is written
    rc = slam_between(s, src->stream, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_work, work.data(), sizeof(PcWork) * work.size(), hipMemcpyHostToDevice, s));
        if (resize) {
            hipLaunchKernelGGL(pc_ancestor_kernel, dim3(grid_for(m)), dim3(256), 0, s, (const double*)d_cdf, (const double*)d_bsum, nb, n, m, u0, d_anc);
            HIP_TRY(hipGetLastError());
            int rcb;
            if ((rcb = pc_launch_gather<T, true>(dst, src, d_work, d_anc, (T)0, 0, (T)(-log((double)m)), s))) return rcb;
            if (anc_out) HIP_TRY(hipMemcpyAsync(anc_out, d_anc, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
            return SLAM_OK;
        }
        return pc_launch_gather<T, false>(dst, src, d_work, nullptr, (T)pend, src->has_pending ? 1 : 0, (T)0, s);
    });
    // the launches have gone out (or dst is in an unknown state): the bookkeeping follows the device
    dst->has_pending = 0;
    dst->pending_shift = 0.0;
    for (int l = 0; l < dst->nl; ++l) {
        if (dst->ltab[l] >= 0) {                 // every slot of buffer cur was just overwritten: plain maps again
            dst->tref[dst->ltab[l]] -= 1;
            dst->ltab[l] = -1;
        }
        dst->lbuf[l] = (int8_t)dst->cur;
        dst->seen[l] = l < cnt ? src->seen[slots[l]] : 0;
    }
    dst->lazy_dirty = 0;
    dst->seed = src->seed;
    dst->step = src->step;
    dst->nresamples = src->nresamples + (resize ? 1 : 0);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));            // (`work` and anc_out are pageable host memory)
    return SLAM_OK;
}

int pc_enter_pair(slam_pf* dst, slam_pf* src) {
    HIP_TRY(hipSetDevice(src->device));
    PF_LEGACY_ENTRY(src);                        // (the bookkeeping comes home; as slam_pf_download leaves the filter)
    PF_LEGACY_ENTRY(dst);
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_pf_get_meta(slam_pf_t h, int64_t out[8], uint8_t* seen) {
    ARG_CHECK(h != nullptr && out != nullptr, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);                          // waits for the queue; step, resample count and `seen` are the host's again
    out[0] = h->n; out[1] = h->n_global; out[2] = h->first; out[3] = h->nl; out[4] = h->dtype;
    out[5] = (int64_t)h->step; out[6] = (int64_t)h->nresamples; out[7] = (int64_t)h->seed;
    if (seen)
        for (int l = 0; l < h->nl; ++l) seen[l] = h->seen[l] ? 1 : 0;
    return SLAM_OK;
}

extern "C" int slam_pf_set_rng(slam_pf_t h, uint64_t seed, uint32_t step) {
    ARG_CHECK(h != nullptr, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    h->seed = seed;
    h->step = step;
    return SLAM_OK;
}

extern "C" int slam_pf_upload(slam_pf_t h, const void* pose, const void* logw, const void* lm, const uint8_t* seen) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK((lm == nullptr) == (seen == nullptr), "lm and seen are given together or not at all");
    ARG_CHECK(h->d_peers == nullptr, "slam_pf_upload needs a filter without peers");
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    const size_t n = (size_t)h->n;
    if (logw) {                                  // the stored values are replaced: a deferred shift is moot
        h->has_pending = 0;
        h->pending_shift = 0.0;
    }
    if (pose) HIP_TRY(hipMemcpyAsync(h->pose[h->pcur], pose, h->esz * 3 * n, hipMemcpyHostToDevice, h->stream));
    if (logw) HIP_TRY(hipMemcpyAsync(h->logw, logw, h->esz * n, hipMemcpyHostToDevice, h->stream));
    if (lm) {                                    // chunk by chunk out of the caller's contiguous [nl][5][n]
        for (int k = 0; k < h->lmtab.nchunks; ++k) {
            const size_t l0 = (size_t)k << h->lmtab.shift;
            const size_t lms = (size_t)h->nl - l0 < ((size_t)1 << h->lmtab.shift) ? (size_t)h->nl - l0 : ((size_t)1 << h->lmtab.shift);
            HIP_TRY(hipMemcpyAsync(h->lmtab.c[h->cur][k], (const char*)lm + h->esz * 5 * n * l0, h->esz * 5 * n * lms, hipMemcpyHostToDevice,
                                   h->stream));
        }
        for (int l = 0; l < h->nl; ++l) {
            if (h->ltab[l] >= 0) {               // every slot of buffer cur is overwritten: plain maps again
                h->tref[h->ltab[l]] -= 1;
                h->ltab[l] = -1;
            }
            h->lbuf[l] = (int8_t)h->cur;
            h->seen[l] = seen[l] ? 1 : 0;
        }
        h->lazy_dirty = 0;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

extern "C" int slam_pf_select(slam_pf_t dst, slam_pf_t src, const int32_t* ids, int cnt, int fill) {
    SLAM_RANGE();
    int rc;
    if ((rc = pc_check_pair(dst, src))) return rc;
    ARG_CHECK(fill == 0 || fill == 1, "fill must be 0 or 1");
    ARG_CHECK(dst->n == src->n, "slam_pf_select needs equal particle counts (slam_pf_resize changes the count)");
    std::vector<int32_t> slots;                  // 0-based
    if (ids == nullptr) {
        for (int l = 0; l < src->nl; ++l) slots.push_back(l);
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
    if ((int)slots.size() > dst->nl) {
        slam_set_error("slam_pf_select: %d landmarks exceed capacity %d", (int)slots.size(), dst->nl);
        return SLAM_E_CAPACITY;
    }
    if ((rc = pc_enter_pair(dst, src))) return rc;
    return dst->dtype == SLAM_F32 ? pc_move<float>(dst, src, slots, fill, false, 0.0, 0.0, nullptr)
                                  : pc_move<double>(dst, src, slots, fill, false, 0.0, 0.0, nullptr);
}

extern "C" int slam_pf_copy(slam_pf_t dst, slam_pf_t src, int fill) {
    int rc;
    if ((rc = pc_check_pair(dst, src))) return rc;
    if (dst->nl < src->nl) {
        slam_set_error("slam_pf_copy: %d landmark slots exceed capacity %d (a smaller destination goes through slam_pf_select)", src->nl, dst->nl);
        return SLAM_E_CAPACITY;
    }
    return slam_pf_select(dst, src, nullptr, 0, fill);
}

extern "C" int slam_pf_resize(slam_pf_t dst, slam_pf_t src, double gmax, double u0, int fill, int32_t* anc) {
    SLAM_RANGE();
    int rc;
    if ((rc = pc_check_pair(dst, src))) return rc;
    ARG_CHECK(fill == 0 || fill == 1, "fill must be 0 or 1");
    ARG_CHECK(u0 >= 0.0 && u0 < 1.0, "u0 must be in [0, 1)");
    ARG_CHECK(std::isfinite(gmax), "gmax is not finite");
    if (dst->nl < src->nl) {
        slam_set_error("slam_pf_resize: %d landmark slots exceed capacity %d", src->nl, dst->nl);
        return SLAM_E_CAPACITY;
    }
    std::vector<int32_t> slots;
    for (int l = 0; l < src->nl; ++l) slots.push_back(l);
    if ((rc = pc_enter_pair(dst, src))) return rc;
    return dst->dtype == SLAM_F32 ? pc_move<float>(dst, src, slots, fill, true, gmax, u0, anc) : pc_move<double>(dst, src, slots, fill, true, gmax, u0, anc);
}

extern "C" int slam_pf_pose_bins(slam_pf_t h, double cell_xy, double cell_phi, int64_t* bins) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr && bins != nullptr, "null argument");
    ARG_CHECK(std::isfinite(cell_xy) && std::isfinite(cell_phi) && cell_xy > 0.0 && cell_phi > 0.0, "the cells must be positive and finite");
    const double ncell = ceil(2.0 * PF_PI / cell_phi);
    ARG_CHECK(ncell <= 2097152.0, "more than 2^21 heading cells");
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    int log2_slots = 0;
    while (((int64_t)1 << log2_slots) < h->n) ++log2_slots;
    log2_slots += 1;                                                     // 2 next_pow2(n) slots: at most half of them fill up
    const size_t o_out = 0, o_set = 256, total = o_set + sizeof(unsigned long long) * ((size_t)1 << log2_slots);
    int rc;
    HIP_TRY(hipStreamSynchronize(h->stream));                            // (the scratch may be replaced)
    if ((rc = pc_workspace(h, total))) return rc;
    char* ws = (char*)h->d_mapws;
    unsigned long long* d_out = (unsigned long long*)(ws + o_out);
    unsigned long long* d_set = (unsigned long long*)(ws + o_set);
    unsigned long long res[2] = {0ull, 0ull};
    HIP_TRY(hipMemsetAsync(d_out, 0, 256, h->stream));
    HIP_TRY(hipMemsetAsync(d_set, 0xff, sizeof(unsigned long long) * ((size_t)1 << log2_slots), h->stream));
    PF_DISPATCH(h,
                hipLaunchKernelGGL(pc_bins_kernel<T>, dim3(grid_for(h->n)), dim3(256), 0, h->stream, (const T*)h->pose[h->pcur], h->n, cell_xy,
                                   cell_phi, (long long)ncell - 1, d_set, log2_slots, d_out),
                hipLaunchKernelGGL(pc_bins_kernel<T>, dim3(grid_for(h->n)), dim3(256), 0, h->stream, (const T*)h->pose[h->pcur], h->n, cell_xy,
                                   cell_phi, (long long)ncell - 1, d_set, log2_slots, d_out));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(res, d_out, sizeof(res), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    ARG_CHECK(res[1] == 0ull, "a pose is not finite or lies 2^20 cells or more from the origin");
    *bins = (int64_t)res[0];
    return SLAM_OK;
}
