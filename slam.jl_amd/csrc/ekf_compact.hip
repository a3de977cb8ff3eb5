// ekf_compact.hip -- map management: landmarks taken out of the state IN PLACE (slam_ekf_remove_landmarks).
//
// Marginalising a landmark out of a Gaussian is deleting its two rows / columns of P and its two entries of x:
//     x <- x[keep],  P <- P[keep, keep]        keep = the surviving state indices, ascending, so keep[i] >= i.
// No arithmetic, so the result is exact; it is a data-movement problem on the tile-major, block-lower storage
// (device_math.h).  Destination entry (r', c') takes source entry (keep[r'], keep[c']).
//
// In place, with a BOUNDED staging buffer and no wait between workgroups inside a launch; stream order alone makes it safe:
//   * the destination column bands are walked in ascending order, in groups [J0, J1) whose tiles fit the staging buffer;
//   * launch A (compact_gather_kernel) forms every destination tile of the group FROM THE MATRIX and writes it to staging.
//     A destination column c' >= J0 E reads source column keep[c'] >= c', i.e. only bands >= J0, and no band >= J0 has been
//     written yet.  The part of a diagonal tile above the diagonal is the mirror of the part below (source (keep[c'], keep[r']),
//     source column keep[r'] >= r' >= J0 E: the same argument);
//   * launch B (compact_store_kernel) copies staging over the group's bands.  The next group's launch A reads bands >= J1 only.
// Nothing below the first removed state index f0 moves: tile rows I < I0 = f0 / E hold rows (and therefore columns) below f0
// only and are skipped, tile rows above I1 = (n_old - 1) / E are padding before and after.  Band J contributes the tile rows
// max(J, I0) .. I1, which are contiguous in memory.  Removing the youngest landmarks therefore moves O(n E) elements, not
// O(n^2).  Destination indices >= n_new are written as +0.0: the vacated tail is padding again.
#include "common.h"
#include "device_math.h"

namespace {

// tiles the schedule moves in the bands [J0, J): band j holds the tile rows max(j, I0) .. I1
__host__ __device__ inline long long compact_tiles_before(int J0, int J, int I0, int I1) {
    long long s = 0;
    const int a = (J < I0 ? J : I0) - J0;                    // bands of [J0, J) left of I0: I1 - I0 + 1 tiles each
    if (a > 0) s += (long long)a * (I1 - I0 + 1);
    const int lo = J0 > I0 ? J0 : I0;                         // bands j of [lo, J): I1 + 1 - j tiles each
    const int cnt = J - lo;
    if (cnt > 0) s += (long long)cnt * (I1 + 1) - ((long long)cnt * (lo + J - 1)) / 2;
    return s;
}

// source element (kr, kc) of the stored triangle, kr >= kc
template <typename T>
__device__ __forceinline__ T compact_fetch(const T* __restrict__ P, const int32_t* __restrict__ keep, int ld, int L, int n_new, int r,
                                           int c) {
    return r < n_new ? P[p_off(ld, L, keep[r], keep[c])] : (T)0;      // (c <= r: c is a surviving index too)
}

// Launch A.  Workgroup (x, y): destination tile (I, J) = (max(J, I0) + x, J0 + y) -> staging.  Lanes walk the rows of a
// destination column: the source rows keep[r'] are runs of consecutive rows (shifted by two per removed landmark above
// them), so a wave reads a few contiguous pieces of one source column.
template <typename T>
__global__ __launch_bounds__(256) void compact_gather_kernel(const T* __restrict__ P, T* __restrict__ stage,
                                                              const int32_t* __restrict__ keep, int ld, int n_new, int I0, int I1,
                                                              int J0) {
    constexpr int L = kTileLog2<T>;                   // tile edge 128 (fp32) / 64 (fp64)
    constexpr int E = 1 << L, m = E - 1;
    const int J = J0 + blockIdx.y;
    const int I = (J > I0 ? J : I0) + blockIdx.x;
    if (I > I1) return;
    T* __restrict__ dst = stage + ((size_t)(compact_tiles_before(J0, J, I0, I1) + blockIdx.x) << (2 * L));
    if (I != J) {
        // a tile below the diagonal: every entry has r' > c'.  Per column the source offset splits into a part of the column
        // alone (kept in LDS) and a part of the row alone (kept in registers).
        __shared__ long long colpart[E];
        const int Tt = ld >> L;
        if ((int)threadIdx.x < E) {
            const int c = (J << L) + threadIdx.x;
            long long cp = -1;                                            // column >= n_new: zeros
            if (c < n_new) {
                const int kc = keep[c], Js = kc >> L;
                cp = (((long long)Js * Tt - (long long)Js * (Js - 1) / 2 - Js) << (2 * L)) + ((long long)(kc & m) << L);
            }
            colpart[threadIdx.x] = cp;
        }
        __syncthreads();
        const int rl = threadIdx.x & m;
        const int r = (I << L) + rl;
        long long rowpart = -1;
        if (r < n_new) {
            const int kr = keep[r];
            rowpart = ((long long)(kr >> L) << (2 * L)) + (kr & m);
        }
        constexpr int cstep = 256 >> L;
#pragma unroll 8
        for (int cl = threadIdx.x >> L; cl < E; cl += cstep) {
            const long long cp = colpart[cl];
            const T v = (rowpart >= 0 && cp >= 0) ? P[cp + rowpart] : (T)0;
            dst[((size_t)cl << L) + rl] = v;
        }
        return;
    }
    // a diagonal tile, stored complete: 32 x 32 blocks; a block above the diagonal is read as its mirror (coalesced) and
    // transposed through LDS, as unpack_kernel does
    __shared__ T sh[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int base = J << L;
    constexpr int S = E >> 5;
    for (int bi = 0; bi < S; ++bi)
        for (int bj = 0; bj < S; ++bj) {
            if (bi >= bj) {
                for (int j = ty; j < 32; j += 8) {
                    const int rl = 32 * bi + tx, cl = 32 * bj + j;
                    const int hi = rl > cl ? rl : cl, lo = rl > cl ? cl : rl;      // (inside a block ON the diagonal: the mirror)
                    dst[((size_t)cl << L) + rl] = compact_fetch(P, keep, ld, L, n_new, base + hi, base + lo);
                }
            } else {
                for (int j = ty; j < 32; j += 8)                                   // element (32 bj + tx, 32 bi + j): below the diagonal
                    sh[j][tx] = compact_fetch(P, keep, ld, L, n_new, base + 32 * bj + tx, base + 32 * bi + j);
                __syncthreads();
                for (int j = ty; j < 32; j += 8)                                   // (r', c') = (32 bi + tx, 32 bj + j) = its mirror
                    dst[((size_t)(32 * bj + j) << L) + 32 * bi + tx] = sh[tx][j];
                __syncthreads();
            }
        }
}

// Launch B.  The same grid: staging tile -> tile (I, J) of the matrix, 16 bytes per lane (both sides are tile aligned).
template <typename T>
__global__ __launch_bounds__(256) void compact_store_kernel(T* __restrict__ P, const T* __restrict__ stage, int ld, int I0, int I1,
                                                             int J0) {
    constexpr int L = kTileLog2<T>;
    const int J = J0 + blockIdx.y;
    const int I = (J > I0 ? J : I0) + blockIdx.x;
    if (I > I1) return;
    const uint4* __restrict__ src = (const uint4*)(stage + ((size_t)(compact_tiles_before(J0, J, I0, I1) + blockIdx.x) << (2 * L)));
    uint4* __restrict__ dst = (uint4*)(P + tile_base(I, J, ld >> L, L));
    constexpr int nvec = (int)((sizeof(T) << (2 * L)) / 16);
#pragma unroll 4
    for (int i = threadIdx.x; i < nvec; i += 256) dst[i] = src[i];
}

// x: entries [f0, n_old) of the compacted vector (zeros from n_new on) into a staging vector; copied back by the caller
template <typename T>
__global__ __launch_bounds__(256) void compact_x_kernel(const T* __restrict__ x, T* __restrict__ xs, const int32_t* __restrict__ keep,
                                                         int f0, int n_new, int n_old) {
    const int i = f0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_old) return;
    xs[i - f0] = i < n_new ? x[keep[i]] : (T)0;
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

template <typename T>
int compact_impl(slam_ekf* h, const int32_t* keep_host, int n_new, int n_old, int f0, int L) {
    const int I0 = f0 >> L, I1 = (n_old - 1) >> L;
    const size_t tile_bytes = sizeof(T) << (2 * L);
    // staging: the <= 256 MiB rule of the state transfers (at least one whole band)
    const long long total = compact_tiles_before(0, I1 + 1, I0, I1);
    long long cap = (long long)(((size_t)256 << 20) / tile_bytes);
    if (cap < I1 - I0 + 1) cap = I1 - I0 + 1;
    if (cap > total) cap = total;
    DevBuf keep_d, xs_d, stage_d;
    HIP_TRY(hipMalloc(&keep_d.p, sizeof(int32_t) * (size_t)n_new));
    HIP_TRY(hipMalloc(&xs_d.p, sizeof(T) * (size_t)(n_old - f0)));
    HIP_TRY(hipMalloc(&stage_d.p, tile_bytes * (size_t)cap));
    const int32_t* keep = (const int32_t*)keep_d.p;
    HIP_TRY(hipMemcpyAsync(keep_d.p, keep_host, sizeof(int32_t) * (size_t)n_new, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(compact_x_kernel<T>, dim3((n_old - f0 + 255) / 256), dim3(256), 0, h->stream, (const T*)h->x, (T*)xs_d.p, keep, f0,
                       n_new, n_old);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync((T*)h->x + f0, xs_d.p, sizeof(T) * (size_t)(n_old - f0), hipMemcpyDeviceToDevice, h->stream));
    for (int J0 = 0; J0 <= I1;) {
        int J1 = J0 + 1;                                         // as many whole bands as fit
        while (J1 <= I1 && compact_tiles_before(J0, J1 + 1, I0, I1) <= cap) ++J1;
        const dim3 grid(I1 - (J0 > I0 ? J0 : I0) + 1, J1 - J0);
        hipLaunchKernelGGL(compact_gather_kernel<T>, grid, dim3(256), 0, h->stream, (const T*)h->P, (T*)stage_d.p, keep, h->ld, n_new, I0,
                           I1, J0);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(compact_store_kernel<T>, grid, dim3(256), 0, h->stream, (T*)h->P, (const T*)stage_d.p, h->ld, I0, I1, J0);
        HIP_TRY(hipGetLastError());
        J0 = J1;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));                   // the staging buffers (and the caller's keep) are released
    return SLAM_OK;
}

}  // namespace

// keep_host[0 .. n_new): the surviving state indices, ascending; f0: the first removed state index; h->N is still the old count
int launch_compact(slam_ekf* h, const int32_t* keep_host, int n_new, int f0) {
    const int n_old = 3 + 2 * h->N;
    if (h->dtype == SLAM_F32) return compact_impl<float>(h, keep_host, n_new, n_old, f0, 7);
    return compact_impl<double>(h, keep_host, n_new, n_old, f0, 6);
}
