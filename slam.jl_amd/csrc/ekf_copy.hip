// ekf_copy.hip -- an EKF state moved between two handles on the device: slam_ekf_copy, slam_ekf_select, slam_ekf_capacity
// (include/slamhip_copy.h states the rule; tests/copy_ref.py runs it literally).
//
//     x'[i] = x[s(i)],  P'[i, j] = P[s(i), s(j)]        s = the identity (copy) or the index map of the chosen landmarks (select)
// No arithmetic: a data-movement problem between two tile-major, block-lower buffers (device_math.h) whose tile rows T = ld / E
// differ, so that tile (I, J) has another block number on either side.
//
// ONE launch moves the matrix and clears what dst held beyond the new state.  Its work items are (tile, slice of 32 columns =
// 16 KiB) over the tiles (I, J), J <= I < Tw, Tw = the tile rows below max(n_old, n'), numbered band after band -- the order in
// which both buffers lie in memory -- and a grid of at most 2048 workgroups (256 CUs x 8 resident workgroups) strides over them;
// one workgroup per tile would be 1.2 million workgroups at N = 50 000 fp64.
//   move_tiles_kernel   (copy)    the slice is 1024 pieces of 16 bytes, four per thread, loaded from src's tile (I, J) and stored
//                                 to dst's tile (I, J): both bases are 32 / 64 KiB aligned.  Non-temporal on both sides (see
//                                 SLAM_COPY_NT).  A tile at or beyond ceil(n' / E) is stored as zeros without a load.
//   gather_tiles_kernel (select)  thread t: row rl = t mod E of the tile, columns 32 u + t / E + k (256 / E).  The lanes of a wave walk
//                                 the rows of ONE destination column: coalesced stores, a wave-uniform source column s(c'), and
//                                 source rows s(r') that are adjacent for the two rows of a landmark and consecutive for sorted ids.
//                                 The source entry is read where it is stored (the lower entry inside a source diagonal tile).
//                                 Inside a destination diagonal tile the thread with r' >= c' writes the entry and its mirror
//                                 from the one value it loaded (p_store_sym); the thread with r' < c' writes nothing.
// OWNERSHIP: every stored offset of dst below Tw has exactly one writing thread (an entry and its mirror inside a diagonal tile:
// the same thread), nothing beyond is written, src is only read.  No LDS, no atomics, no private scratch, all offsets 64-bit.
// ids reach the device through dst's pinned observation staging (h_idf -> idfbuf, the path slam_ekf_update's idf takes): grow-only,
// guarded by the staging event, and nothing else is allocated.
#include <vector>

#include "common.h"
#include "../../include/slamhip_copy.h"
#include "device_math.h"

// Stores (and the copy's loads) of the matrix: 1 = non-temporal, 0 = plain.  dst is usually read next by a gating sweep (its
// packed side array only) and a down-date (the whole matrix, far larger than the caches at the sizes where the time matters).
// DESIGN 5.9 has the measurement behind the default.
#ifndef SLAM_COPY_NT
#define SLAM_COPY_NT 1
#endif

namespace {

constexpr int MOVE_THREADS = 256;
constexpr int MOVE_GRID_MAX = 2048;
constexpr int SLICE_COLS = 32;           // columns of a slice: 32 E elements = 16 KiB in both dtypes

typedef unsigned vec4u __attribute__((ext_vector_type(4)));

template <typename V>
__device__ __forceinline__ V mv_load(const V* p) {
#if SLAM_COPY_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

template <typename V>
__device__ __forceinline__ void mv_store(V v, V* p) {
#if SLAM_COPY_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// source state index of destination index i (select); i < n'
__device__ __forceinline__ int src_index(const int32_t* __restrict__ ids, int i) {
    return i < 3 ? i : 3 + 2 * (ids[(i - 3) >> 1] - 1) + ((i - 3) & 1);
}

template <typename T>
__global__ __launch_bounds__(MOVE_THREADS) void move_tiles_kernel(T* __restrict__ Pd, int ldd, const T* __restrict__ Ps, int lds, int Tw,
                                                                   int Tn, long long items) {
    constexpr int L = kTileLog2<T>;
    constexpr int S = (1 << L) / SLICE_COLS;                            // slices of a tile
    constexpr int PIECES = SLICE_COLS * (int)sizeof(T) * (1 << L) / 16;   // 16-byte pieces of a slice: 1024
    constexpr int PER = PIECES / MOVE_THREADS;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const long long q = w / S;
        const int u = (int)(w - q * S);
        int I, J;
        tile_of(q, Tw, &I, &J);
        vec4u* __restrict__ d = reinterpret_cast<vec4u*>(Pd + tile_base(I, J, ldd >> L, L)) + (size_t)u * PIECES + threadIdx.x;
        vec4u v[PER];
        if (I < Tn) {
            const vec4u* __restrict__ s = reinterpret_cast<const vec4u*>(Ps + tile_base(I, J, lds >> L, L)) + (size_t)u * PIECES + threadIdx.x;
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = mv_load(s + k * MOVE_THREADS);
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = vec4u{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) mv_store(v[k], d + k * MOVE_THREADS);
    }
}

template <typename T>
__global__ __launch_bounds__(MOVE_THREADS) void gather_tiles_kernel(T* __restrict__ Pd, int ldd, const T* __restrict__ Ps, int lds,
                                                                     const int32_t* __restrict__ ids, int nn, int Tw, long long items) {
    constexpr int L = kTileLog2<T>;
    constexpr int E = 1 << L;
    constexpr int S = E / SLICE_COLS;
    constexpr int CSTEP = MOVE_THREADS >> L;                             // columns the workgroup covers at a time
    const int rl = threadIdx.x & (E - 1), c_sub = threadIdx.x >> L;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const long long q = w / S;
        const int u = (int)(w - q * S);
        int I, J;
        tile_of(q, Tw, &I, &J);
        const int r = (I << L) + rl;
        const int a = r < nn ? src_index(ids, r) : -1;
        const int c0 = (J << L) + u * SLICE_COLS + c_sub;
        if (I != J) {
            // three passes, each of independent accesses: the source columns, the values, the stores (one dependent chain of
            // index load -> value load -> store per column kept a thread at two loads in flight)
            constexpr int K = SLICE_COLS / CSTEP;
            int b[K];
            T v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int c = c0 + k * CSTEP;
                b[k] = (a >= 0 && c < nn) ? src_index(ids, c) : -1;
            }
#pragma unroll
            for (int k = 0; k < K; ++k)
                v[k] = b[k] < 0 ? (T)0 : ((a >> L) >= (b[k] >> L) ? Ps[p_off(lds, L, a, b[k])] : Ps[p_off(lds, L, b[k], a)]);
#pragma unroll
            for (int k = 0; k < K; ++k) mv_store(v[k], Pd + p_off(ldd, L, r, c0 + k * CSTEP));
        } else {
            for (int k = 0; k < SLICE_COLS / CSTEP; ++k) {
                const int c = c0 + k * CSTEP;
                if (r < c) continue;                                      // the mirror: written by the owner of (c, r)
                T v = (T)0;
                if (a >= 0) {                                             // (c <= r < n')
                    const int b = src_index(ids, c);
                    const int hi = a > b ? a : b, lo = a > b ? b : a;   // one source tile row: the LOWER entry; else the stored one
                    v = (a >> L) == (b >> L) ? Ps[p_off(lds, L, hi, lo)]
                                             : ((a >> L) > (b >> L) ? Ps[p_off(lds, L, a, b)] : Ps[p_off(lds, L, b, a)]);
                }
                p_store_sym(Pd, ldd, L, r, c, v);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void gather_x_kernel(T* __restrict__ xd, const T* __restrict__ xs, const int32_t* __restrict__ ids, int nn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nn) xd[i] = xs[src_index(ids, i)];
}

// the panel workspace's rows >= n must be zero for the down-date (ekf_api.hip does the same when an upload shrinks the map)
int zero_panels_of(slam_ekf* h) {
    if (!h->kcap) return SLAM_OK;
    HIP_TRY(hipMemsetAsync(h->PHt, 0, sizeof(double) * (size_t)h->npad * h->kcap, h->stream));
    HIP_TRY(hipMemsetAsync(h->Kd, 0, sizeof(double) * (size_t)h->npad * h->kcap, h->stream));
    HIP_TRY(hipMemsetAsync(h->W1, 0, h->esz * (size_t)h->npad * 2 * h->kcap, h->stream));
    HIP_TRY(hipMemsetAsync(h->W2, 0, h->esz * (size_t)h->npad * 2 * h->kcap, h->stream));
    return SLAM_OK;
}

// ids -> dst's device index buffer through its pinned staging, as stage_obs (ekf_api.hip) sends an update's idf
int stage_ids(slam_ekf* dst, const int32_t* ids, int cnt) {
    if (dst->stage_pending) {                                            // the pinned buffer may still feed an earlier copy
        HIP_TRY(hipEventSynchronize(dst->stage_ev));
        dst->stage_pending = 0;
    }
    memcpy(dst->h_idf, ids, sizeof(int32_t) * (size_t)cnt);
    HIP_TRY(hipMemcpyAsync(dst->idfbuf, dst->h_idf, sizeof(int32_t) * (size_t)cnt, hipMemcpyHostToDevice, dst->stream));
    HIP_TRY(hipEventRecord(dst->stage_ev, dst->stream));
    dst->stage_pending = 1;
    return SLAM_OK;
}

// everything enqueued on dst's stream; N2: the landmarks dst receives; ids == nullptr: a copy
template <typename T>
int move_impl(slam_ekf* dst, const slam_ekf* src, const int32_t* ids, int N2) {
    constexpr int L = kTileLog2<T>;
    constexpr int E = 1 << L;
    const int nn = 3 + 2 * N2, n_old = 3 + 2 * dst->N;
    const int Td = dst->ld >> L;
    int Tw = ((nn > n_old ? nn : n_old) + E - 1) >> L;
    if (Tw > Td) Tw = Td;
    const int Tn = (nn + E - 1) >> L;
    const long long items = (long long)Tw * (Tw + 1) / 2 * (E / SLICE_COLS);
    const unsigned grid = (unsigned)(items < MOVE_GRID_MAX ? items : MOVE_GRID_MAX);
    int rc;
    if (N2 < dst->N && (rc = zero_panels_of(dst))) return rc;
    if (ids) {
        if (N2 > 0 && (rc = stage_ids(dst, ids, N2))) return rc;
        const int32_t* d_ids = dst->idfbuf;
        hipLaunchKernelGGL(gather_x_kernel<T>, dim3((nn + 255) / 256), dim3(256), 0, dst->stream, (T*)dst->x, (const T*)src->x, d_ids, nn);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(gather_tiles_kernel<T>, dim3(grid), dim3(MOVE_THREADS), 0, dst->stream, (T*)dst->P, dst->ld, (const T*)src->P,
                           src->ld, d_ids, nn, Tw, items);
    } else {
        HIP_TRY(hipMemcpyAsync(dst->x, src->x, sizeof(T) * (size_t)nn, hipMemcpyDeviceToDevice, dst->stream));
        hipLaunchKernelGGL(move_tiles_kernel<T>, dim3(grid), dim3(MOVE_THREADS), 0, dst->stream, (T*)dst->P, dst->ld, (const T*)src->P,
                           src->ld, Tw, Tn, items);
    }
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

// the part copy and select share: validated by the caller; ordered against src's stream by slam_between (common.h)
int move_between(slam_ekf* dst, slam_ekf* src, const int32_t* ids, int N2) {
    int rc;
    if (src->pending_status && (rc = slam_ekf_sync(src))) return rc;     // src's deferred status; dst untouched
    HIP_TRY(hipSetDevice(dst->device));
    if (ids && N2 > 0 && (rc = ensure_obs_capacity(dst, N2))) return rc;   // the index buffer and its staging: grow only
    return slam_between(dst->stream, src->stream, [&]() -> int {
        const int rcm = dst->dtype == SLAM_F32 ? move_impl<float>(dst, src, ids, N2) : move_impl<double>(dst, src, ids, N2);
        if (rcm) return rcm;
        // the launches have gone out: the host side follows the device at once, whatever the event calls behind them return
        dst->N = N2;
        dst->grid_force = 1;                                             // the grid belongs to dst's old means
        dst->pmax_valid = 0;                                             // ... and the variance bound to its old matrix
        return launch_side_rebuild(dst);                                 // the packed 2 x 2 diagonal blocks follow the matrix
    });
}

int check_pair(slam_ekf* dst, slam_ekf* src) {
    ARG_CHECK(dst != nullptr && src != nullptr, "null handle");
    ARG_CHECK(dst != src, "source and destination are one handle");
    ARG_CHECK(dst->dtype == src->dtype, "the two states differ in dtype");
    ARG_CHECK(dst->device == src->device, "the two states live on different devices");
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_ekf_capacity(slam_ekf_t h, int* max_landmarks) {
    ARG_CHECK(h != nullptr && max_landmarks != nullptr, "null argument");
    *max_landmarks = h->maxN;
    return SLAM_OK;
}

extern "C" int slam_ekf_copy(slam_ekf_t dst, slam_ekf_t src) {
    SLAM_RANGE();
    int rc;
    if ((rc = check_pair(dst, src))) return rc;
    if (src->N > dst->maxN) {
        slam_set_error("copy: %d landmarks exceed capacity %d", src->N, dst->maxN);
        return SLAM_E_CAPACITY;
    }
    return move_between(dst, src, nullptr, src->N);
}

extern "C" int slam_ekf_select(slam_ekf_t dst, slam_ekf_t src, const int32_t* ids, int cnt) {
    SLAM_RANGE();
    int rc;
    if ((rc = check_pair(dst, src))) return rc;
    ARG_CHECK(cnt >= 0, "cnt < 0");
    ARG_CHECK(cnt == 0 || ids != nullptr, "ids is null");
    {
        std::vector<char> seen((size_t)src->N + 1, 0);
        for (int i = 0; i < cnt; ++i) {
            ARG_CHECK(ids[i] >= 1 && ids[i] <= src->N, "landmark id out of range");
            ARG_CHECK(!seen[ids[i]], "duplicate landmark id");
            seen[ids[i]] = 1;
        }
    }
    if (cnt > dst->maxN) {
        slam_set_error("select: %d landmarks exceed capacity %d", cnt, dst->maxN);
        return SLAM_E_CAPACITY;
    }
    static const int32_t none = 0;                                        // cnt == 0: still a select (nothing is read through it)
    return move_between(dst, src, cnt > 0 ? ids : &none, cnt);
}
