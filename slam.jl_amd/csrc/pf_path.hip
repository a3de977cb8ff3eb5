// pf_path.hip -- per-particle trajectory history of the particle filter (include/slamhip_path.h): a ring of pose snapshots and
// ancestor arrays on the device, the composition of the resamplings between two records, and the read-outs that follow the
// current particles back through the ring.  libslamhip_path.so.
//
//   record     ONE launch: a flat copy of the live poses (3 n values) into the slot and, when a resampling is pending, of the
//              pending map (n int32) into the slot's ancestor array; thread 0 writes the slot's device flag.  16-byte units when
//              n is a multiple of 4 (every slot of both rings is then 16-byte aligned), 4-byte units otherwise.
//   compose    pend'[p] = pend[anc[p]]: a 4-byte gather, out of place.
//   mean       the hot one: n L gathers of 12 (fp32) to 24 (fp64) bytes, plus 4 where a record has ancestors.  One thread per
//              particle keeps (w, index) in registers and walks the records newest to oldest; a wave's 64 indices are those of
//              64 CONSECUTIVE particles.  Systematic resampling yields non-decreasing ancestors and a composition of
//              non-decreasing maps is non-decreasing (tests/test_path_ref_cpu.py checks both on tests/resample_ref.py), so the
//              indices of a wave stay sorted at every record: its gathers fall into a few neighbouring cache lines, equal
//              neighbours into the same one (the memory pipeline serves lanes of one instruction that share a line with one
//              request: nothing to do by hand).  The walk is a chain of L dependent gathers, so a record's loads are issued one
//              iteration ahead of its arithmetic, the ancestor word first; nothing in the loop synchronises the waves: per
//              record a wave reduces its four products (path_wave_sum_split: 7 exchanges instead of 24) and writes ONE line
//              [record][wave][4] of partial sums; the lines of row L hold sum w.  A second kernel folds the lines of a row in
//              a fixed order.  No atomics: two calls give the same bits.  (What was measured on the way: DESIGN 5.3c.)
//   survivors  a backward sweep with two byte arrays: a marked particle stores a plain 1 into its ancestor's byte (colliding
//              stores write the same value), the same kernel counts the marks it reads (integer atomics: exact in any order).
//              One launch per slot whose ancestors are not the identity; the host repeats the count across identity slots.
//   trace      one thread per requested particle walks the slots; `best` finds the particle on the device (as pf_best_kernel of
//              pf_map.hip does) and feeds its index to the same kernel.
//
// Every index that a gather uses was written by compose (which clamps what it reads to 0 .. n - 1) or copied from such an array;
// a slot's ancestor array is read only when its flag says it was written.  The walkers clamp once more all the same: a gather out
// of bounds must not depend on a buffer being what the host believes it to be.
#include <cmath>

#include "pf_internal.h"
#include "../../include/slamhip_path.h"

struct slam_pf_path {
    slam_pf* h;                      // borrowed
    int cap;
    void* d_pose;                    // [cap][3][n] in the filter's dtype
    int32_t* d_anc;                  // [cap][n]
    int32_t* d_flag;                 // [cap] device copy of has_anc (written by the record kernel, read by the walkers)
    std::vector<char> has_anc;       // [cap]
    int32_t* d_pend[2];              // [n] the composed ancestors of the resamplings since the last record
    int pcur, has_pend;
    int64_t nrec, nres;              // records ever made, resamplings seen
    long long* d_which;              // [2] the particle `best` / `mean` found
    unsigned long long* d_cnt;       // [cap] the survivors' counts
    void* d_ws;                      // grow-only scratch of the read-outs
    size_t ws_bytes;
};

namespace {

constexpr int PATH_WG = 256;
constexpr int PATH_MAXTRACE = SLAM_PF_PATH_MAXTRACE;

// record: dst_pose[0 .. np) <- pose, dst_anc[0 .. na) <- pend (na == 0: nothing pending), in units of V
template <typename V>
__global__ __launch_bounds__(PATH_WG) void pf_path_record_kernel(const V* __restrict__ pose, V* __restrict__ dst_pose, int64_t np,
                                                                 const V* __restrict__ pend, V* __restrict__ dst_anc, int64_t na,
                                                                 int32_t* __restrict__ flag, int32_t has) {
    const int64_t i = (int64_t)blockIdx.x * PATH_WG + threadIdx.x;
    if (i < np) dst_pose[i] = pose[i];
    else if (i - np < na) dst_anc[i - np] = pend[i - np];
    if (i == 0) *flag = has;
}

// pend'[p] = pend[anc[p]] (pend == nullptr: anc[p]); an ancestor outside 0 .. n - 1 counts as p, as in pf_evidence_gather_kernel
__global__ __launch_bounds__(PATH_WG) void pf_path_compose_kernel(const int32_t* __restrict__ anc, const int32_t* __restrict__ pend,
                                                                  int32_t* __restrict__ dst, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * PATH_WG + threadIdx.x;
    if (p >= n) return;
    int64_t a = anc[p];
    if (a < 0 || a >= n) a = p;                      // (pf_ancestor_kernel writes 0 .. n - 1)
    dst[p] = pend ? pend[a] : (int32_t)a;
}

__device__ __forceinline__ int64_t path_clamp(int64_t a, int64_t n, int64_t keep) { return a >= 0 && a < n ? a : keep; }

// the particle with the largest log-weight as stored after the shift `pend`, lowest index on a tie (pf_best_kernel of pf_map.hip)
template <typename T>
__global__ __launch_bounds__(1024) void pf_path_best_kernel(const T* __restrict__ logw, int64_t n, T pend, long long* __restrict__ best) {
    __shared__ double sv[16];
    __shared__ long long si[16];
    double bv = -__builtin_inf();
    long long bi = (long long)n;
    for (int64_t p = threadIdx.x; p < n; p += 1024) {
        const double v = (double)(T)(logw[p] - pend);
        if (v > bv || (v == bv && p < bi)) { bv = v; bi = p; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const long long oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k)
            if (sv[k] > bv || (sv[k] == bv && si[k] < bi)) { bv = sv[k]; bi = si[k]; }
        *best = bi < (long long)n ? bi : 0;              // (every log-weight NaN: particle 0)
    }
}

// out[c][t][3]: the path of current particle ids[c] (ids == nullptr: the one particle *which), one thread per particle
template <typename T>
__global__ __launch_bounds__(PATH_WG) void pf_path_trace_kernel(const T* __restrict__ ring, const int32_t* __restrict__ ring_anc,
                                                                const int32_t* __restrict__ flag, const int32_t* __restrict__ pend,
                                                                const long long* __restrict__ ids, const long long* __restrict__ which,
                                                                int cnt, int64_t n, int cap, int newest, int L,
                                                                double* __restrict__ out) {
    const int c = blockIdx.x * PATH_WG + threadIdx.x;
    if (c >= cnt) return;
    const int64_t p = path_clamp(ids ? (int64_t)ids[c] : (int64_t)*which, n, 0);
    int64_t idx = pend ? path_clamp(pend[p], n, p) : p;
    int slot = newest;
    for (int t = L - 1; t >= 0; --t) {
        const T* __restrict__ ps = ring + (size_t)slot * 3 * (size_t)n;
        double* __restrict__ o = out + ((size_t)c * (size_t)L + (size_t)t) * 3;
        o[0] = (double)ps[idx]; o[1] = (double)ps[(size_t)n + idx]; o[2] = (double)ps[2 * (size_t)n + idx];
        if (t > 0 && flag[slot]) idx = path_clamp(ring_anc[(size_t)slot * (size_t)n + idx], n, idx);
        slot = slot == 0 ? cap - 1 : slot - 1;
    }
}

// the sums of a wave in a fixed order: a butterfly (every lane ends with the same bits); the N chains are independent and interleave
template <int N>
__device__ __forceinline__ void path_wave_sum(double (&a)[N]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] += __shfl_xor(a[k], off);
}

// The N sums of a wave (N a power of two, at most 64) with N - 1 + (6 - log2 N) exchanges instead of 6 N: while more than one
// value is live a lane keeps half of them and hands the other half to its partner, which keeps those (the upper lane of a pair
// the upper half).  Lane l ends with the total of sum l >> (6 - log2 N) in a[0]; the order of the additions is fixed.
template <int N>
__device__ __forceinline__ void path_wave_sum_split(double (&a)[N], int lane) {
    int m = N;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        if (m > 1) {
            m >>= 1;
            const bool upper = (lane & off) != 0;
#pragma unroll
            for (int k = 0; k < N / 2; ++k)
                if (k < m) {
                    const double give = upper ? a[k] : a[k + m], keep = upper ? a[k + m] : a[k];
                    a[k] = keep + __shfl_xor(give, off);
                }
        } else {
            a[0] += __shfl_xor(a[0], off);
        }
    }
}

// part[(row * nlines + line) * 4 + k], one line per WAVE: row t < L the sums {w x, w y, w sin phi, w cos phi} over the wave's
// particles of their ancestors at record t, row L {w, 0, 0, 0}.  The loads of record t - 1 (its ancestor word first: the walk
// waits for nothing else) are issued before the arithmetic of record t, whose values arrived an iteration ago.
template <typename T>
__global__ __launch_bounds__(PATH_WG) void pf_path_mean_kernel(const T* __restrict__ logw, const long long* __restrict__ which,
                                                               const T* __restrict__ ring, const int32_t* __restrict__ ring_anc,
                                                               const int32_t* __restrict__ flag, const int32_t* __restrict__ pend,
                                                               int64_t n, int cap, int newest, int L, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const size_t nlines = (size_t)gridDim.x * (PATH_WG / 64), line = (size_t)blockIdx.x * (PATH_WG / 64) + (threadIdx.x >> 6);
    const int64_t p = (int64_t)blockIdx.x * PATH_WG + threadIdx.x;
    const bool ok = p < n;
    const double lmax = (double)logw[path_clamp((int64_t)*which, n, 0)];
    const double w = ok ? exp((double)logw[p] - lmax) : 0.0;
    int64_t idx = ok ? (pend ? path_clamp(pend[p], n, p) : p) : 0;
    {                                                    // row L: sum w
        double a[1] = {w};
        path_wave_sum<1>(a);
        if (lane < 4) part[((size_t)L * nlines + line) * 4 + lane] = lane == 0 ? a[0] : 0.0;
    }
    int slot = newest;
    bool step = L > 1 && flag[slot] != 0;                // uniform: the walk from this record back goes through its ancestors
    const T* __restrict__ ps = ring + (size_t)slot * 3 * (size_t)n;
    int32_t anc = step && ok ? ring_anc[(size_t)slot * (size_t)n + idx] : 0;
    T x = ok ? ps[idx] : (T)0, y = ok ? ps[(size_t)n + idx] : (T)0, phi = ok ? ps[2 * (size_t)n + idx] : (T)0;
    for (int t = L - 1; t >= 0; --t) {
        const int64_t nidx = step ? path_clamp(anc, n, idx) : idx;
        const int nslot = slot == 0 ? cap - 1 : slot - 1;
        bool nstep = false;
        int32_t nanc = 0;
        T nx = (T)0, ny = (T)0, nphi = (T)0;
        if (t > 0) {                                     // uniform
            nstep = t > 1 && flag[nslot] != 0;
            const T* __restrict__ pn = ring + (size_t)nslot * 3 * (size_t)n;
            if (nstep && ok) nanc = ring_anc[(size_t)nslot * (size_t)n + nidx];
            if (ok) { nx = pn[nidx]; ny = pn[(size_t)n + nidx]; nphi = pn[2 * (size_t)n + nidx]; }
        }
        double sn, cs;
        sincos((double)phi, &sn, &cs);
        double a[4] = {w * (double)x, w * (double)y, w * sn, w * cs};       // (a lane beyond n: w = 0 and zeros)
        path_wave_sum_split<4>(a, lane);
        if ((lane & 15) == 0) part[((size_t)t * nlines + line) * 4 + (lane >> 4)] = a[0];
        x = nx; y = ny; phi = nphi; anc = nanc; step = nstep; idx = nidx; slot = nslot;
    }
}

// out[row][k] = the lines of a row in a fixed order: thread i adds the lines i, i + 256, ... in turn, then a butterfly inside the
// wave and the four waves in index order.  grid: L + 1 rows
__global__ __launch_bounds__(PATH_WG) void pf_path_fold_kernel(const double* __restrict__ part, int nlines, double* __restrict__ out) {
    __shared__ double s_red[PATH_WG / 64][4];
    const int row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = threadIdx.x; g < nlines; g += PATH_WG) {
        const double* __restrict__ line = part + ((size_t)row * nlines + g) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += line[k];
    }
    path_wave_sum<4>(a);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) s_red[wave][k] = a[k];
    __syncthreads();
    if (threadIdx.x < 4)
        out[(size_t)row * 4 + threadIdx.x] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

// survivors, the start: every current particle marks where it sits at the newest record
__global__ __launch_bounds__(PATH_WG) void pf_path_mark_kernel(const int32_t* __restrict__ pend, uint8_t* __restrict__ mark, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * PATH_WG + threadIdx.x;
    if (p >= n) return;
    mark[pend ? path_clamp(pend[p], n, p) : p] = 1;
}

// survivors, one record: count the marks of `mark` into *count and, with anc != nullptr, mark their ancestors in `prev`
__global__ __launch_bounds__(PATH_WG) void pf_path_sweep_kernel(const uint8_t* __restrict__ mark, const int32_t* __restrict__ anc,
                                                                uint8_t* __restrict__ prev, int64_t n,
                                                                unsigned long long* __restrict__ count) {
    __shared__ unsigned s_cnt[PATH_WG / 64];
    const int64_t q = (int64_t)blockIdx.x * PATH_WG + threadIdx.x;
    const bool on = q < n && mark[q] != 0;
    if (on && anc) prev[path_clamp(anc[q], n, q)] = 1;
    unsigned c = on ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned s = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
        if (s) atomicAdd(count, (unsigned long long)s);
    }
}

int path_live(const slam_pf_path* ph) {
    ARG_CHECK(ph != nullptr && ph->h != nullptr, "null path object");
    ARG_CHECK(ph->h->d_peers == nullptr && ph->h->n == ph->h->n_global,
              "the path history supports only a filter that lives wholly on one shard, without peers");
    return SLAM_OK;
}

inline int64_t path_len(const slam_pf_path* ph) { return ph->nrec < ph->cap ? ph->nrec : ph->cap; }
inline int path_newest(const slam_pf_path* ph) { return (int)((ph->nrec - 1) % ph->cap); }
inline int grid_of(int64_t items) { return (int)((items + PATH_WG - 1) / PATH_WG); }

// a read-out begins: the object is live, a record exists, the filter is out of the auto mode
int path_enter(slam_pf_path* ph) {
    const int rc = path_live(ph);
    if (rc) return rc;
    ARG_CHECK(ph->nrec > 0, "no record has been made yet");
    HIP_TRY(hipSetDevice(ph->h->device));
    PF_LEGACY_ENTRY(ph->h);
    return SLAM_OK;
}

int path_workspace(slam_pf_path* ph, size_t bytes) {
    if (bytes <= ph->ws_bytes) return SLAM_OK;
    if (ph->d_ws) (void)hipFree(ph->d_ws);
    ph->d_ws = nullptr;
    ph->ws_bytes = 0;
    bytes = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc(&ph->d_ws, bytes));
    ph->ws_bytes = bytes;
    return SLAM_OK;
}

// the paths of cnt particles (d_ids, or the one in d_which) into d_out[cnt][L][3]; enqueued
int path_launch_trace(slam_pf_path* ph, const long long* d_ids, int cnt, double* d_out) {
    slam_pf* h = ph->h;
    const int32_t* pend = ph->has_pend ? ph->d_pend[ph->pcur] : nullptr;
    const int L = (int)path_len(ph), newest = path_newest(ph);
#define PATH_TRACE()                                                                                                            \
    hipLaunchKernelGGL(pf_path_trace_kernel<T>, dim3(grid_of(cnt)), dim3(PATH_WG), 0, h->stream, (const T*)ph->d_pose,          \
                       (const int32_t*)ph->d_anc, (const int32_t*)ph->d_flag, pend, d_ids, (const long long*)ph->d_which, cnt,  \
                       h->n, ph->cap, newest, L, d_out)
    PF_DISPATCH(h, PATH_TRACE(), PATH_TRACE());
#undef PATH_TRACE
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int path_launch_best(slam_pf_path* ph, double pend_shift) {
    slam_pf* h = ph->h;
    PF_DISPATCH(h,
                hipLaunchKernelGGL(pf_path_best_kernel<T>, dim3(1), dim3(1024), 0, h->stream, (const T*)h->logw, h->n, (T)pend_shift, ph->d_which),
                hipLaunchKernelGGL(pf_path_best_kernel<T>, dim3(1), dim3(1024), 0, h->stream, (const T*)h->logw, h->n, (T)pend_shift, ph->d_which));
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

void path_free(slam_pf_path* ph) {
    void* devs[] = {ph->d_pose, ph->d_anc, ph->d_flag, ph->d_pend[0], ph->d_pend[1], ph->d_which, ph->d_cnt, ph->d_ws};
    for (void* d : devs)
        if (d) (void)hipFree(d);
    delete ph;
}

}  // namespace

extern "C" int slam_pf_path_create(slam_pf_path_t* out, slam_pf_t h, int cap) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr && h != nullptr, "null argument");
    *out = nullptr;
    ARG_CHECK(cap >= 1, "a path history needs at least one slot");
    ARG_CHECK(h->n == h->n_global, "the path history needs the whole filter on this shard (sharded filters are not supported)");
    ARG_CHECK(h->d_peers == nullptr, "the path history does not support a filter with peers attached");
    HIP_TRY(hipSetDevice(h->device));
    slam_pf_path* ph = new slam_pf_path();
    ph->h = h;
    ph->cap = cap;
    ph->d_pose = nullptr;
    ph->d_anc = ph->d_flag = ph->d_pend[0] = ph->d_pend[1] = nullptr;
    ph->d_which = nullptr;
    ph->d_cnt = nullptr;
    ph->d_ws = nullptr;
    ph->ws_bytes = 0;
    ph->pcur = ph->has_pend = 0;
    ph->nrec = ph->nres = 0;
    ph->has_anc.assign((size_t)cap, 0);
    const size_t n = (size_t)h->n, slots = (size_t)cap;
    auto alloc = [](void** p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 16); };
    hipError_t e = alloc(&ph->d_pose, slots * 3 * n * h->esz);
    if (e == hipSuccess) e = alloc((void**)&ph->d_anc, slots * n * sizeof(int32_t));
    if (e == hipSuccess) e = alloc((void**)&ph->d_flag, slots * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemsetAsync(ph->d_flag, 0, slots * sizeof(int32_t), h->stream);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) e = alloc((void**)&ph->d_pend[b], n * sizeof(int32_t));
    if (e == hipSuccess) e = alloc((void**)&ph->d_which, 2 * sizeof(long long));
    if (e == hipSuccess) e = alloc((void**)&ph->d_cnt, slots * sizeof(unsigned long long));
    if (e != hipSuccess) {
        slam_set_error("slam_pf_path_create: %s", hipGetErrorString(e));
        path_free(ph);
        return e == hipErrorOutOfMemory ? SLAM_E_NOMEM : SLAM_E_HIP;
    }
    *out = ph;
    return SLAM_OK;
}

extern "C" int slam_pf_path_destroy(slam_pf_path_t ph) {
    ARG_CHECK(ph != nullptr, "null path object");
    if (ph->h) {
        (void)hipSetDevice(ph->h->device);
        (void)hipStreamSynchronize(ph->h->stream);
    }
    path_free(ph);
    return SLAM_OK;
}

extern "C" int slam_pf_path_record(slam_pf_path_t ph) {
    SLAM_RANGE();
    const int rc = path_live(ph);
    if (rc) return rc;
    slam_pf* h = ph->h;
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    const size_t n = (size_t)h->n;
    const int slot = (int)(ph->nrec % ph->cap);
    const char* src = (const char*)h->pose[h->pcur];
    char* dst = (char*)ph->d_pose + (size_t)slot * 3 * n * h->esz;
    const char* pend = (const char*)ph->d_pend[ph->pcur];
    char* danc = (char*)(ph->d_anc + (size_t)slot * n);
    const size_t pose_bytes = 3 * n * h->esz, anc_bytes = ph->has_pend ? n * sizeof(int32_t) : 0;
    if (n % 4 == 0) {                                // every slot of both rings starts on a 16-byte boundary
        const int64_t np = (int64_t)(pose_bytes / 16), na = (int64_t)(anc_bytes / 16);
        hipLaunchKernelGGL(pf_path_record_kernel<uint4>, dim3(grid_of(np + na > 0 ? np + na : 1)), dim3(PATH_WG), 0, h->stream,
                           (const uint4*)src, (uint4*)dst, np, (const uint4*)pend, (uint4*)danc, na, ph->d_flag + slot,
                           (int32_t)ph->has_pend);
    } else {
        const int64_t np = (int64_t)(pose_bytes / 4), na = (int64_t)(anc_bytes / 4);
        hipLaunchKernelGGL(pf_path_record_kernel<uint32_t>, dim3(grid_of(np + na)), dim3(PATH_WG), 0, h->stream,
                           (const uint32_t*)src, (uint32_t*)dst, np, (const uint32_t*)pend, (uint32_t*)danc, na, ph->d_flag + slot,
                           (int32_t)ph->has_pend);
    }
    HIP_TRY(hipGetLastError());
    ph->has_anc[(size_t)slot] = (char)ph->has_pend;
    ph->has_pend = 0;
    ph->nrec += 1;
    return SLAM_OK;
}

extern "C" int slam_pf_path_resample(slam_pf_path_t ph, double gmax, double u0) {
    SLAM_RANGE();
    int rc = path_live(ph);
    if (rc) return rc;
    slam_pf* h = ph->h;
    if ((rc = slam_pf_resample_local(h, gmax, u0))) return rc;      // fills h->d_anc before its lazy and its eager branch
    hipLaunchKernelGGL(pf_path_compose_kernel, dim3(grid_of(h->n)), dim3(PATH_WG), 0, h->stream, (const int32_t*)h->d_anc,
                       (const int32_t*)(ph->has_pend ? ph->d_pend[ph->pcur] : nullptr), ph->d_pend[ph->pcur ^ 1], h->n);
    HIP_TRY(hipGetLastError());
    ph->pcur ^= 1;
    ph->has_pend = 1;
    ph->nres += 1;
    return SLAM_OK;
}

extern "C" int slam_pf_path_info(slam_pf_path_t ph, int64_t out[4]) {
    const int rc = path_live(ph);
    if (rc) return rc;
    ARG_CHECK(out != nullptr, "null argument");
    out[0] = path_len(ph);
    out[1] = ph->nrec;
    out[2] = ph->cap;
    out[3] = ph->nres;
    return SLAM_OK;
}

extern "C" int slam_pf_path_get(slam_pf_path_t ph, int k, double* pose, int32_t* anc, int* has_anc) {
    SLAM_RANGE();
    int rc = path_live(ph);
    if (rc) return rc;
    ARG_CHECK(ph->nrec > 0, "no record has been made yet");
    ARG_CHECK(k >= 0 && k < path_len(ph), "record index out of range");
    slam_pf* h = ph->h;
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    const size_t n = (size_t)h->n;
    const int slot = (int)((ph->nrec - 1 - k) % ph->cap);
    const bool has = ph->has_anc[(size_t)slot] != 0;
    std::vector<char> raw;
    if (pose) {
        raw.resize(3 * n * h->esz);
        HIP_TRY(hipMemcpyAsync(raw.data(), (const char*)ph->d_pose + (size_t)slot * 3 * n * h->esz, raw.size(), hipMemcpyDeviceToHost,
                               h->stream));
    }
    if (anc && has)
        HIP_TRY(hipMemcpyAsync(anc, ph->d_anc + (size_t)slot * n, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (pose) {
        if (h->dtype == SLAM_F32)
            for (size_t i = 0; i < 3 * n; ++i) pose[i] = (double)((const float*)raw.data())[i];
        else
            memcpy(pose, raw.data(), raw.size());
    }
    if (anc && !has)
        for (size_t p = 0; p < n; ++p) anc[p] = (int32_t)p;
    if (has_anc) *has_anc = has ? 1 : 0;
    return SLAM_OK;
}

extern "C" int slam_pf_path_trace(slam_pf_path_t ph, const int64_t* ids, int cnt, double* out) {
    SLAM_RANGE();
    int rc = path_live(ph);
    if (rc) return rc;
    ARG_CHECK(ids != nullptr && out != nullptr, "null argument");
    ARG_CHECK(cnt >= 1 && cnt <= PATH_MAXTRACE, "a trace takes 1 .. 4096 particles");
    for (int c = 0; c < cnt; ++c) ARG_CHECK(ids[c] >= 0 && ids[c] < ph->h->n, "particle index out of range");
    if ((rc = path_enter(ph))) return rc;
    slam_pf* h = ph->h;
    const size_t L = (size_t)path_len(ph);
    const size_t out_bytes = sizeof(double) * 3 * L * (size_t)cnt, id_bytes = sizeof(long long) * (size_t)cnt;
    if ((rc = path_workspace(ph, out_bytes + id_bytes))) return rc;
    double* d_out = (double*)ph->d_ws;
    long long* d_ids = (long long*)(d_out + 3 * L * (size_t)cnt);
    static_assert(sizeof(long long) == sizeof(int64_t), "ids are copied as they are");
    HIP_TRY(hipMemcpyAsync(d_ids, ids, id_bytes, hipMemcpyHostToDevice, h->stream));
    if ((rc = path_launch_trace(ph, d_ids, cnt, d_out))) return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

extern "C" int slam_pf_path_best(slam_pf_path_t ph, int64_t* idx, double* out) {
    SLAM_RANGE();
    int rc = path_live(ph);
    if (rc) return rc;
    ARG_CHECK(out != nullptr, "null argument");
    if ((rc = path_enter(ph))) return rc;
    slam_pf* h = ph->h;
    const size_t out_bytes = sizeof(double) * 3 * (size_t)path_len(ph);
    if ((rc = path_workspace(ph, out_bytes))) return rc;
    const double pend = h->has_pending ? h->pending_shift : 0.0;      // read, not taken: the query changes nothing
    if ((rc = path_launch_best(ph, pend))) return rc;
    if ((rc = path_launch_trace(ph, nullptr, 1, (double*)ph->d_ws))) return rc;
    long long which = 0;
    HIP_TRY(hipMemcpyAsync(&which, ph->d_which, sizeof(which), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(out, ph->d_ws, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (idx) *idx = (int64_t)which;
    return SLAM_OK;
}

extern "C" int slam_pf_path_mean(slam_pf_path_t ph, double* out) {
    SLAM_RANGE();
    int rc = path_live(ph);
    if (rc) return rc;
    ARG_CHECK(out != nullptr, "null argument");
    if ((rc = path_enter(ph))) return rc;
    slam_pf* h = ph->h;
    const int L = (int)path_len(ph), newest = path_newest(ph);
    const int nwg = grid_of(h->n), nlines = nwg * (PATH_WG / 64);
    const size_t rows = (size_t)L + 1;
    const size_t part_bytes = sizeof(double) * 4 * rows * (size_t)nlines, sum_bytes = sizeof(double) * 4 * rows;
    if ((rc = path_workspace(ph, part_bytes + sum_bytes))) return rc;
    double* d_part = (double*)ph->d_ws;
    double* d_sum = d_part + 4 * rows * (size_t)nlines;
    const int32_t* pend = ph->has_pend ? ph->d_pend[ph->pcur] : nullptr;
    if ((rc = path_launch_best(ph, 0.0))) return rc;              // the largest STORED log-weight: a deferred shift cancels
#define PATH_MEAN()                                                                                                              \
    hipLaunchKernelGGL(pf_path_mean_kernel<T>, dim3(nwg), dim3(PATH_WG), 0, h->stream, (const T*)h->logw,                       \
                       (const long long*)ph->d_which, (const T*)ph->d_pose, (const int32_t*)ph->d_anc, (const int32_t*)ph->d_flag, \
                       pend, h->n, ph->cap, newest, L, d_part)
    PF_DISPATCH(h, PATH_MEAN(), PATH_MEAN());
#undef PATH_MEAN
    hipLaunchKernelGGL(pf_path_fold_kernel, dim3((unsigned)rows), dim3(PATH_WG), 0, h->stream, (const double*)d_part, nlines, d_sum);
    HIP_TRY(hipGetLastError());
    std::vector<double> s(4 * rows);
    HIP_TRY(hipMemcpyAsync(s.data(), d_sum, sum_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double W = s[4 * (size_t)L];
    for (int t = 0; t < L; ++t) {
        const double* r = &s[4 * (size_t)t];
        out[4 * t] = r[0] / W;
        out[4 * t + 1] = r[1] / W;
        out[4 * t + 2] = atan2(r[2], r[3]);
        out[4 * t + 3] = hypot(r[2], r[3]) / W;
    }
    return SLAM_OK;
}

extern "C" int slam_pf_path_survivors(slam_pf_path_t ph, int64_t* out) {
    SLAM_RANGE();
    int rc = path_live(ph);
    if (rc) return rc;
    ARG_CHECK(out != nullptr, "null argument");
    if ((rc = path_enter(ph))) return rc;
    slam_pf* h = ph->h;
    const int L = (int)path_len(ph);
    const size_t n = (size_t)h->n;
    const size_t mark_bytes = (n + 15) & ~(size_t)15;
    if ((rc = path_workspace(ph, 2 * mark_bytes))) return rc;
    uint8_t* mark[2] = {(uint8_t*)ph->d_ws, (uint8_t*)ph->d_ws + mark_bytes};
    int cur = 0;
    HIP_TRY(hipMemsetAsync(ph->d_cnt, 0, sizeof(unsigned long long) * (size_t)L, h->stream));
    HIP_TRY(hipMemsetAsync(mark[cur], 0, mark_bytes, h->stream));
    hipLaunchKernelGGL(pf_path_mark_kernel, dim3(grid_of(h->n)), dim3(PATH_WG), 0, h->stream,
                       (const int32_t*)(ph->has_pend ? ph->d_pend[ph->pcur] : nullptr), mark[cur], h->n);
    // mark[cur] holds the marks of record t.  A launch at t counts them and, where slot t has ancestors, marks record t - 1 in the
    // other array; across a slot whose ancestors are the identity the marks, and with them the count, stay what they are:
    // counted[t] says which records a launch counted, `fresh` that the marks have not been counted yet
    std::vector<char> counted((size_t)L, 0);
    bool fresh = true;
    int slot = path_newest(ph);
    for (int t = L - 1; t >= 0; --t) {
        const bool step = t > 0 && ph->has_anc[(size_t)slot];
        if (step || fresh) {
            if (step) HIP_TRY(hipMemsetAsync(mark[cur ^ 1], 0, mark_bytes, h->stream));
            hipLaunchKernelGGL(pf_path_sweep_kernel, dim3(grid_of(h->n)), dim3(PATH_WG), 0, h->stream, (const uint8_t*)mark[cur],
                               (const int32_t*)(step ? ph->d_anc + (size_t)slot * n : nullptr), mark[cur ^ 1], h->n, ph->d_cnt + t);
            counted[(size_t)t] = 1;
            if (step) cur ^= 1;
            fresh = step;
        }
        slot = slot == 0 ? ph->cap - 1 : slot - 1;
    }
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> c((size_t)L);
    HIP_TRY(hipMemcpyAsync(c.data(), ph->d_cnt, sizeof(unsigned long long) * (size_t)L, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int t = L - 1; t >= 0; --t) out[t] = counted[(size_t)t] ? (int64_t)c[(size_t)t] : out[t + 1];
    return SLAM_OK;
}
