// pf_map.hip -- read-outs of the FastSLAM state: the weighted map (slam_pf_map_sums / slam_pf_get_map) and one particle's
// whole record (slam_pf_get_particle).  DESIGN section "FastSLAM map read-out".
//
// The reduction is ONE pass over the landmark records where they are: landmark l's record of particle p sits in buffer
// lbuf[l] at slot tab[ltab[l]][p] (slot p without a table), exactly what the sweep of the filter step reads, so a filter that
// lives wholly on this shard is neither materialised nor changed in any way.  The pass is bound by HBM (20 B per particle and
// landmark in fp32, 40 B in fp64, plus 4 B per table entry), the arithmetic is a dozen fp64 operations per record.
//
//   grid (slabs of MAP_SLAB particles, groups of `lg` work-list entries), 256 threads
//   a workgroup forms the weights w = exp((double)(T)(logw - pending shift)) of its slab ONCE (16 per thread, in registers)
//   and walks its entries with them: ten fp64 accumulators per thread, xor butterfly inside the wave, the four waves through
//   LDS in wave order, one line of ten doubles per (entry, slab) into `part`; pf_map_fold_kernel adds the slabs' lines in a
//   fixed order (lane i takes slabs i, i + 64, ..., then the butterfly).  No floating-point atomics anywhere: the result is
//   the same bit for bit from call to call.  Longest chain of additions: 16 (thread) + 6 + 3 (workgroup) + slabs / 64 + 6.
//
// Two instantiations per dtype: VEC reads the five rows with 16-byte loads (four fp32 / two fp64 particles per load; records
// without a table, n a multiple of the vector width so that every row is 16-byte aligned), the other one goes through the
// ancestor table particle by particle (lane i takes particle base + i: after systematic resampling a table is non-decreasing
// in p, so a wave's 64 slots are a short ascending run of the source row -- mostly the same cache lines a plain read takes).
// The host sorts the entries into the two kinds; the pose (row 0 of the result) has a small kernel of its own.
#include <math.h>
#include <string.h>

#include <vector>

#include "pf_internal.h"

namespace {

constexpr int MAP_SLAB = 4096;          // particles per workgroup
constexpr int MAP_PER = MAP_SLAB / 256; // ... per thread
constexpr int MAP_LG_MAX = 8;           // entries per workgroup (the weights are formed once for all of them)
constexpr int MAP_COLS = 10;
// work list: three words per entry {landmark (0-based), (table + 1) | buffer << 8 | seen << 9, output row}
constexpr int32_t MW_TAB = 0xff, MW_BUF = 1 << 8, MW_SEEN = 1 << 9;

template <typename T> struct MapVec;
template <> struct MapVec<float> { typedef float4 type; static constexpr int W = 4; };
template <> struct MapVec<double> { typedef double2 type; static constexpr int W = 2; };

template <typename T>
__device__ __forceinline__ T vec_get(const typename MapVec<T>::type& v, int i);
template <>
__device__ __forceinline__ float vec_get<float>(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
template <>
__device__ __forceinline__ double vec_get<double>(const double2& v, int i) { return i == 0 ? v.x : v.y; }

// a record is in use: Pxx > 0.  (Pxx = -1 marks an empty slot of the unknown-correspondence mode, the all-zero record a
// landmark never seen in the known-correspondence mode.  slam_pf_init_landmarks with var = 0 gives used records with
// Pxx == 0: those count when the landmark is `seen`.)
template <typename T>
__device__ __forceinline__ bool map_used(T pxx, bool seen) { return pxx > (T)0 || (seen && pxx == (T)0); }

// (`in`: 1.0 for a record in use, 0.0 otherwise -- then with w = 0 and zeros for the values)
__device__ __forceinline__ void map_acc(double (&a)[MAP_COLS], double w, double mx, double my, double pxx, double pxy, double pyy,
                                        double in = 1.0) {
    const double wx = w * mx, wy = w * my;
    a[0] += w; a[1] += wx; a[2] += wy; a[3] += wx * mx; a[4] += wx * my; a[5] += wy * my;
    a[6] += w * pxx; a[7] += w * pxy; a[8] += w * pyy; a[9] += in;
}

// the workgroup's ten sums -> part[line]: butterfly inside each wave, then wave 0 + 1 + 2 + 3 by ten threads
__device__ __forceinline__ void map_block_store(double (&a)[MAP_COLS], double (*sh)[MAP_COLS], double* __restrict__ line) {
#pragma unroll
    for (int i = 0; i < MAP_COLS; ++i)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a[i] += __shfl_xor(a[i], off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                     // (the previous entry's line has been read)
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < MAP_COLS; ++i) sh[wave][i] = a[i];
    __syncthreads();
    if (threadIdx.x < MAP_COLS) line[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// row 0 of the result, the pose: W, w x, w y, w x^2, w x y, w y^2, w sin(phi), w cos(phi), 0, n_local
template <typename T>
__global__ __launch_bounds__(256) void pf_map_pose_kernel(const T* __restrict__ logw, const T* __restrict__ pose, int64_t n, T pend,
                                                           double* __restrict__ part) {
    __shared__ double sh[4][MAP_COLS];
    double a[MAP_COLS];
#pragma unroll
    for (int i = 0; i < MAP_COLS; ++i) a[i] = 0.0;
    for (int j = 0; j < MAP_PER; ++j) {
        const int64_t p = (int64_t)blockIdx.x * MAP_SLAB + (int64_t)j * 256 + threadIdx.x;
        if (p < n) {
            const double w = exp((double)(T)(logw[p] - pend));
            double sn, cs;
            sincos((double)pose[2 * n + p], &sn, &cs);
            map_acc(a, w, (double)pose[p], (double)pose[n + p], sn, cs, 0.0);      // (w sin, w cos in columns 6 and 7, zeros in 8)
        }
    }
    map_block_store(a, sh, part + (size_t)blockIdx.x * MAP_COLS);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256, 4) void pf_map_kernel(LmView<T> lv, const int32_t* __restrict__ tabs, const T* __restrict__ logw,
                                                         int64_t n, T pend,
                                                         const int32_t* __restrict__ work, int e0, int e1, int lg, int nslabs,
                                                      double* __restrict__ part) {
    typedef typename MapVec<T>::type V;
    constexpr int W = VEC ? MapVec<T>::W : 1;
    constexpr int CH = MAP_PER / W;                     // loads per row and thread
    __shared__ double sh[4][MAP_COLS];
    const int64_t slab0 = (int64_t)blockIdx.x * MAP_SLAB;
    // particle of (chunk j, element i): slab0 + (j * 256 + thread) * W + i -- a wave's load is one contiguous piece of a row
    double w[MAP_PER];
#pragma unroll
    for (int j = 0; j < CH; ++j) {
        const int64_t p = slab0 + ((int64_t)j * 256 + threadIdx.x) * W;
        if constexpr (VEC) {
            if (p < n) {                                 // (n is a multiple of W: the whole vector is inside)
                const V lw = *reinterpret_cast<const V*>(logw + p);
#pragma unroll
                for (int i = 0; i < W; ++i) w[j * W + i] = exp((double)(T)(vec_get<T>(lw, i) - pend));
            } else {
#pragma unroll
                for (int i = 0; i < W; ++i) w[j * W + i] = 0.0;
            }
        } else {
            w[j] = p < n ? exp((double)(T)(logw[p] - pend)) : 0.0;
        }
    }
    const int ea = e0 + blockIdx.y * lg, eb = ea + lg < e1 ? ea + lg : e1;
    for (int e = ea; e < eb; ++e) {
        const int32_t l = work[3 * e], meta = work[3 * e + 1], row_out = work[3 * e + 2];
        double a[MAP_COLS];
#pragma unroll
        for (int i = 0; i < MAP_COLS; ++i) a[i] = 0.0;
        const T* __restrict__ rows = lv.rows((meta & MW_BUF) ? 1 : 0, l, n);
        const bool seen = (meta & MW_SEEN) != 0;
        // No branch between the loads and the sums: a particle past the end reads particle 0's record with weight 0, a record
        // not in use enters as zeros with weight 0 -- a branch on Pxx (or on p < n) would put the other rows' loads behind the
        // arrival of that row and keep the chunks' loads from overlapping.
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                // (a workgroup-uniform test per PAIR of chunks: it bounds the loads in flight to ten 16-byte loads per lane --
                //  without it the compiler hoists all of the slab's loads and spills)
                if (slab0 + (int64_t)(j & ~1) * 256 * W >= n) continue;
                const int64_t p = slab0 + ((int64_t)j * 256 + threadIdx.x) * W;
                const bool valid = p < n;                        // (n is a multiple of W: the whole vector is inside)
                const int64_t q = valid ? p : 0;
                const V mx = *reinterpret_cast<const V*>(rows + q);
                const V my = *reinterpret_cast<const V*>(rows + (size_t)n + q);
                const V pxx = *reinterpret_cast<const V*>(rows + 2 * (size_t)n + q);
                const V pxy = *reinterpret_cast<const V*>(rows + 3 * (size_t)n + q);
                const V pyy = *reinterpret_cast<const V*>(rows + 4 * (size_t)n + q);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const bool in = valid && map_used<T>(vec_get<T>(pxx, i), seen);
                    map_acc(a, in ? w[j * W + i] : 0.0, in ? (double)vec_get<T>(mx, i) : 0.0, in ? (double)vec_get<T>(my, i) : 0.0,
                            in ? (double)vec_get<T>(pxx, i) : 0.0, in ? (double)vec_get<T>(pxy, i) : 0.0,
                            in ? (double)vec_get<T>(pyy, i) : 0.0, in ? 1.0 : 0.0);
                }
            }
        } else {
            const int t = meta & MW_TAB;
            const int32_t* __restrict__ tab = t ? tabs + (size_t)(t - 1) * (size_t)n : nullptr;
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                if (slab0 + (int64_t)(j & ~3) * 256 >= n) continue;          // (workgroup-uniform, per four chunks: as above)
                const int64_t p = slab0 + (int64_t)j * 256 + threadIdx.x;
                const bool valid = p < n;
                const int64_t q = valid ? p : 0;
                const int64_t s = tab ? (int64_t)tab[q] : q;
                const T mx = rows[s], my = rows[(size_t)n + s], pxx = rows[2 * (size_t)n + s], pxy = rows[3 * (size_t)n + s],
                        pyy = rows[4 * (size_t)n + s];
                const bool in = valid && map_used<T>(pxx, seen);
                map_acc(a, in ? w[j] : 0.0, in ? (double)mx : 0.0, in ? (double)my : 0.0, in ? (double)pxx : 0.0, in ? (double)pxy : 0.0,
                        in ? (double)pyy : 0.0, in ? 1.0 : 0.0);
            }
        }
        map_block_store(a, sh, part + ((size_t)row_out * nslabs + blockIdx.x) * MAP_COLS);
    }
}

// out[row][k] = the slabs' lines added in a fixed order: lane i takes slabs i, i + 64, ...; then the butterfly.  One wave per row.
__global__ __launch_bounds__(64) void pf_map_fold_kernel(const double* __restrict__ part, int nslabs, double* __restrict__ out) {
    const size_t row = blockIdx.x;
    for (int k = 0; k < MAP_COLS; ++k) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nslabs; b += 64) s += part[(row * nslabs + b) * MAP_COLS + k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (threadIdx.x == 0) out[row * MAP_COLS + k] = s;
    }
}

// the local particle with the largest log-weight as stored after the pending shift, lowest index on a tie.  One workgroup.
template <typename T>
__global__ __launch_bounds__(1024) void pf_best_kernel(const T* __restrict__ logw, int64_t n, T pend, long long* __restrict__ best) {
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

// ONE particle's record through the tables: out = {index, log-weight, x, y, phi, nl x 5 record values}
template <typename T>
__global__ __launch_bounds__(256) void pf_particle_kernel(LmView<T> lv, const int32_t* __restrict__ tabs, const T* __restrict__ logw,
                                                           const T* __restrict__ pose, int64_t n, int nl, T pend,
                                                           const int32_t* __restrict__ meta, long long idx,
                                                           const long long* __restrict__ which, double* __restrict__ out) {
    const int64_t p = idx >= 0 ? (int64_t)idx : (int64_t)*which;      // (idx < 0: what pf_best_kernel found)
    if (p < 0 || p >= n) return;
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l == 0) {
        out[0] = (double)p;
        out[1] = (double)(T)(logw[p] - pend);
        out[2] = (double)pose[p]; out[3] = (double)pose[n + p]; out[4] = (double)pose[2 * n + p];
    }
    if (meta == nullptr || l >= nl) return;
    const int32_t m = meta[l];
    const int t = m & MW_TAB;
    const int64_t s = t ? (int64_t)tabs[(size_t)(t - 1) * (size_t)n + p] : p;
    const T* __restrict__ rows = lv.rows((m & MW_BUF) ? 1 : 0, l, n);
#pragma unroll
    for (int c = 0; c < 5; ++c) out[5 + 5 * (size_t)l + c] = (double)rows[(size_t)c * (size_t)n + s];
}

// grow-only scratch of the read-outs (partials, work list, results), kept with the handle
int map_workspace(slam_pf* h, size_t bytes) {
    if (bytes <= h->mapws_bytes) return SLAM_OK;
    if (h->d_mapws) (void)hipFree(h->d_mapws);
    h->d_mapws = nullptr;
    h->mapws_bytes = 0;
    bytes = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc(&h->d_mapws, bytes));
    h->mapws_bytes = bytes;
    return SLAM_OK;
}

inline int32_t map_meta(const slam_pf* h, int l) {
    return (int32_t)(h->ltab[l] + 1) | (h->lbuf[l] ? MW_BUF : 0) | (h->seen[l] ? MW_SEEN : 0);
}

// The remote records of a filter with peers come home first (collective; its tables hold global ids).  A filter that lives
// wholly on this shard is read where it is.
int map_enter(slam_pf* h, bool records) {
    HIP_TRY(hipSetDevice(h->device));
    PF_LEGACY_ENTRY(h);
    if (records && h->n != h->n_global) return pf_materialise(h);
    return SLAM_OK;
}

int map_sums_impl(slam_pf* h, const int32_t* ids, int cnt, double* out) {
    const int rce = map_enter(h, true);
    if (rce) return rce;
    const int rows = cnt + 1;
    const int64_t n = h->n;
    const int nslabs = (int)((n + MAP_SLAB - 1) / MAP_SLAB);
    const int vw = h->dtype == SLAM_F32 ? 4 : 2;
    const bool vec_ok = n % vw == 0;
    // work list: the table kind first, then the vector kind
    std::vector<int32_t> work((size_t)3 * rows);
    int ng = 0, ntab = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < cnt; ++i) {
            const int l = ids ? ids[i] - 1 : i;
            const bool vec = vec_ok && h->ltab[l] < 0;
            if (vec != (pass == 1)) continue;
            work[3 * (size_t)ng] = l; work[3 * (size_t)ng + 1] = map_meta(h, l); work[3 * (size_t)ng + 2] = i + 1;
            ++ng;
            ntab += pass == 0;
        }
    const size_t part_bytes = sizeof(double) * MAP_COLS * (size_t)rows * nslabs, out_bytes = sizeof(double) * MAP_COLS * (size_t)rows;
    const size_t work_bytes = sizeof(int32_t) * 3 * (size_t)rows;
    { const int rcw = map_workspace(h, part_bytes + out_bytes + work_bytes); if (rcw) return rcw; }
    double* d_part = (double*)h->d_mapws;
    double* d_out = d_part + (size_t)MAP_COLS * rows * nslabs;
    int32_t* d_work = (int32_t*)(d_out + (size_t)MAP_COLS * rows);
    HIP_TRY(hipMemcpyAsync(d_work, work.data(), work_bytes, hipMemcpyHostToDevice, h->stream));
    const double pend = h->has_pending ? h->pending_shift : 0.0;      // read, not taken: the query changes nothing
    // entries per workgroup: as many as keep about 2048 workgroups in the launch (at most MAP_LG_MAX), and a grid.y that fits
    auto group = [&](int entries) {
        int lg = (int)((int64_t)entries * nslabs / 2048);
        lg = lg < 1 ? 1 : (lg > MAP_LG_MAX ? MAP_LG_MAX : lg);
        while ((entries + lg - 1) / lg > 65535) lg *= 2;
        return lg;
    };
    PF_DISPATCH(h,
                hipLaunchKernelGGL(pf_map_pose_kernel<T>, dim3(nslabs), dim3(256), 0, h->stream, (const T*)h->logw,
                                   (const T*)h->pose[h->pcur], n, (T)pend, d_part),
                hipLaunchKernelGGL(pf_map_pose_kernel<T>, dim3(nslabs), dim3(256), 0, h->stream, (const T*)h->logw,
                                   (const T*)h->pose[h->pcur], n, (T)pend, d_part));
    HIP_TRY(hipGetLastError());
    for (int kind = 0; kind < 2; ++kind) {
        const int e0 = kind == 0 ? 0 : ntab, e1 = kind == 0 ? ntab : cnt;
        if (e1 == e0) continue;
        const int lg = group(e1 - e0);
        const dim3 grid(nslabs, (e1 - e0 + lg - 1) / lg);
        if (kind == 0)
            PF_DISPATCH(h,
                        hipLaunchKernelGGL((pf_map_kernel<T, false>), grid, dim3(256), 0, h->stream, LmView<T>{h->d_lmtab},
                                           (const int32_t*)h->d_tab[h->tside], (const T*)h->logw, n, (T)pend,
                                           (const int32_t*)d_work, e0, e1, lg, nslabs, d_part),
                        hipLaunchKernelGGL((pf_map_kernel<T, false>), grid, dim3(256), 0, h->stream, LmView<T>{h->d_lmtab},
                                           (const int32_t*)h->d_tab[h->tside], (const T*)h->logw, n, (T)pend,
                                           (const int32_t*)d_work, e0, e1, lg, nslabs, d_part));
        else
            PF_DISPATCH(h,
                        hipLaunchKernelGGL((pf_map_kernel<T, true>), grid, dim3(256), 0, h->stream, LmView<T>{h->d_lmtab},
                                           (const int32_t*)h->d_tab[h->tside], (const T*)h->logw, n, (T)pend,
                                           (const int32_t*)d_work, e0, e1, lg, nslabs, d_part),
                        hipLaunchKernelGGL((pf_map_kernel<T, true>), grid, dim3(256), 0, h->stream, LmView<T>{h->d_lmtab},
                                           (const int32_t*)h->d_tab[h->tside], (const T*)h->logw, n, (T)pend,
                                           (const int32_t*)d_work, e0, e1, lg, nslabs, d_part));
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pf_map_fold_kernel, dim3(rows), dim3(64), 0, h->stream, (const double*)d_part, nslabs, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

}  // namespace

#define MAP_CHECK_IDS(h, ids, cnt, out)                                                                   \
    do {                                                                                              \
        ARG_CHECK((h) != nullptr && (out) != nullptr, "null argument");                                 \
        if ((ids) == nullptr) (cnt) = (h)->nl;                                                        \
        ARG_CHECK((cnt) >= 0, "cnt < 0");                                                             \
        if (ids)                                                                                      \
            for (int i_ = 0; i_ < (cnt); ++i_) ARG_CHECK((ids)[i_] >= 1 && (ids)[i_] <= (h)->nl, "landmark id out of range"); \
    } while (0)

/* The local sums of the weighted map: out[(1 + cnt) * 10], row 0 the pose, row 1 + i landmark ids[i] (1-based; NULL: all nl,
 * cnt ignored).  Synchronises; a filter wholly on this shard is read where it is and not changed; with peers attached the
 * call is collective (the remote records come home first). */
extern "C" int slam_pf_map_sums(slam_pf_t h, const int32_t* ids, int cnt, double* out) {
    SLAM_RANGE();
    MAP_CHECK_IDS(h, ids, cnt, out);
    return map_sums_impl(h, ids, cnt, out);
}

/* The moment-matched Gaussian of every asked landmark; the whole filter on this shard. */
extern "C" int slam_pf_get_map(slam_pf_t h, const int32_t* ids, int cnt, double* out) {
    SLAM_RANGE();
    MAP_CHECK_IDS(h, ids, cnt, out);
    ARG_CHECK(h->n == h->n_global, "slam_pf_get_map needs the whole filter on this shard (a sharded filter adds slam_pf_map_sums over its ranks)");
    std::vector<double> s((size_t)MAP_COLS * (cnt + 1));
    const int rc = map_sums_impl(h, ids, cnt, s.data());
    if (rc) return rc;
    const double W = s[0];
    for (int i = 0; i < cnt; ++i) {
        const double* r = &s[(size_t)MAP_COLS * (i + 1)];
        double* o = out + (size_t)8 * i;
        for (int k = 0; k < 8; ++k) o[k] = 0.0;
        if (!(r[0] > 0.0) || !(W > 0.0)) continue;
        const double mx = r[1] / r[0], my = r[2] / r[0];
        o[0] = r[0] / W; o[1] = mx; o[2] = my;
        o[3] = r[6] / r[0] + (r[3] / r[0] - mx * mx);
        o[4] = r[7] / r[0] + (r[4] / r[0] - mx * my);
        o[5] = r[8] / r[0] + (r[5] / r[0] - my * my);
        o[6] = r[9];
    }
    return SLAM_OK;
}

/* One local particle: idx, or -1 for the one with the largest log-weight (lowest index on a tie). */
extern "C" int slam_pf_get_particle(slam_pf_t h, int64_t idx, int64_t* gid, double* logw, double pose[3], double* lm) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK(idx >= -1 && idx < h->n, "particle index out of range");
    const int rce = map_enter(h, lm != nullptr);
    if (rce) return rce;
    const int nl = h->nl;
    const size_t out_doubles = 5 + (size_t)5 * nl;
    { const int rcw = map_workspace(h, sizeof(double) * out_doubles + 16 + sizeof(int32_t) * (size_t)nl); if (rcw) return rcw; }
    double* d_out = (double*)h->d_mapws;
    long long* d_which = (long long*)(d_out + out_doubles);
    int32_t* d_meta = (int32_t*)(d_which + 2);
    std::vector<int32_t> meta;
    const double pend = h->has_pending ? h->pending_shift : 0.0;
    if (idx < 0) {
        PF_DISPATCH(h,
                    hipLaunchKernelGGL(pf_best_kernel<T>, dim3(1), dim3(1024), 0, h->stream, (const T*)h->logw, h->n, (T)pend, d_which),
                    hipLaunchKernelGGL(pf_best_kernel<T>, dim3(1), dim3(1024), 0, h->stream, (const T*)h->logw, h->n, (T)pend, d_which));
        HIP_TRY(hipGetLastError());
    }
    if (lm) {
        meta.resize(nl);
        for (int l = 0; l < nl; ++l) meta[l] = map_meta(h, l);
        HIP_TRY(hipMemcpyAsync(d_meta, meta.data(), sizeof(int32_t) * (size_t)nl, hipMemcpyHostToDevice, h->stream));
    }
    const dim3 grid(lm ? (nl + 255) / 256 : 1);
    PF_DISPATCH(h,
                hipLaunchKernelGGL(pf_particle_kernel<T>, grid, dim3(256), 0, h->stream, LmView<T>{h->d_lmtab},
                                   (const int32_t*)h->d_tab[h->tside], (const T*)h->logw, (const T*)h->pose[h->pcur], h->n, nl, (T)pend,
                                   (const int32_t*)(lm ? d_meta : nullptr), (long long)idx, (const long long*)d_which, d_out),
                hipLaunchKernelGGL(pf_particle_kernel<T>, grid, dim3(256), 0, h->stream, LmView<T>{h->d_lmtab},
                                   (const int32_t*)h->d_tab[h->tside], (const T*)h->logw, (const T*)h->pose[h->pcur], h->n, nl, (T)pend,
                                   (const int32_t*)(lm ? d_meta : nullptr), (long long)idx, (const long long*)d_which, d_out));
    HIP_TRY(hipGetLastError());
    std::vector<double> head(5);
    HIP_TRY(hipMemcpyAsync(head.data(), d_out, sizeof(double) * 5, hipMemcpyDeviceToHost, h->stream));
    if (lm) HIP_TRY(hipMemcpyAsync(lm, d_out + 5, sizeof(double) * 5 * (size_t)nl, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (gid) *gid = h->first + (int64_t)head[0];
    if (logw) *logw = head[1];
    if (pose) { pose[0] = head[2]; pose[1] = head[3]; pose[2] = head[4]; }
    return SLAM_OK;
}
