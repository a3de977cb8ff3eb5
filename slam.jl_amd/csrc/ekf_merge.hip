// ekf_merge.hip -- map management: duplicate landmarks found (slam_ekf_find_duplicates) and fused (slam_ekf_merge_landmarks).
//
// FIND.  Landmarks a < b are duplicates when the Mahalanobis distance of their difference is inside the gate:
//     delta = m_b - m_a,   D = P_aa + P_bb - P_ab - P_ab'   (symmetrised),   D > 0  and  delta' inv(D) delta < gate.
// There are N (N - 1) / 2 pairs and their cross blocks P_ab are the whole matrix, so a pair is first tested on the means and the
// packed diagonal blocks (Pside) alone: for a positive semi-definite joint covariance D <= 2 (P_aa + P_bb), hence
//     d2 >= |delta|^2 / (2 (tr P_aa + tr P_bb)),
// and a pair with |delta|^2 >= 2 gate (tr P_aa + tr P_bb) cannot be inside the gate.  Only the survivors read their four
// cross entries.  With a < b every entry P[f_b + i, f_a + j] has row > column, so it exists in the block-lower storage as it
// stands (p_off) whichever tiles the two landmarks' rows and columns fall into (one, two or four of them when a landmark
// straddles a tile edge); P_ab is the transpose of that stored block.
//
// MERGE.  "a_p and b_p are one point" for the pairs p of a call is ONE linear measurement with rows +I2 at a_p, -I2 at b_p,
// value 0 and noise Rc: the reference's Cholesky-form update (src/ekf.jl:67-75) with k = 2 cnt <= 16.  The front half here
// (merge_factor_kernel, merge_panel_kernel) forms S, C = inv(chol(S)), g = C C' v, W1 = PHt C and x += PHt g in double; the
// down-date P -= W1 W1' is launch_downdate on the plain 16-column panel, and the removal of the b_p is launch_compact.
#include <algorithm>
#include <math.h>

#include "common.h"
#include "device_math.h"

namespace {

constexpr int FD_TA = 64;        // landmarks a of a workgroup's block of the (a, b) triangle: LDS
constexpr int FD_TB = 256;       // landmarks b: one per thread, registers
// the cheap bound is compared with a relative margin far above the rounding of its six double operations, so that rounding can
// never reject a pair the exact test would keep
constexpr double FD_SLACK = 1.0 + 1.0 / (double)(1 << 30);

template <typename T>
__global__ __launch_bounds__(FD_TB) void find_dup_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld,
                                                          const T* __restrict__ side, int side_n, int N, double gate,
                                                          int2* __restrict__ pairs, unsigned long long cap,
                                                          unsigned long long* __restrict__ cursor) {
    constexpr int L = kTileLog2<T>;
    const int a0 = blockIdx.y * FD_TA, b0 = blockIdx.x * FD_TB;          // 0-based landmarks
    const int bend = b0 + FD_TB < N ? b0 + FD_TB : N;
    if (a0 >= bend - 1) return;                                          // no pair a < b in this block
    __shared__ double s_x[FD_TA], s_y[FD_TA], s_g[FD_TA], s_00[FD_TA], s_10[FD_TA], s_11[FD_TA];
    const int tid = threadIdx.x;
    const int na = N - a0 < FD_TA ? N - a0 : FD_TA;
    if (tid < na) {
        const int a = a0 + tid;
        const double p00 = (double)side[a], p10 = (double)side[(size_t)side_n + a], p11 = (double)side[(size_t)2 * side_n + a];
        s_x[tid] = (double)x[3 + 2 * a];
        s_y[tid] = (double)x[4 + 2 * a];
        s_g[tid] = 2.0 * gate * (p00 + p11) * FD_SLACK;
        s_00[tid] = p00; s_10[tid] = p10; s_11[tid] = p11;
    }
    const int b = b0 + tid;
    const bool valid = b < N;
    double xb = 0.0, yb = 0.0, b00 = 0.0, b10 = 0.0, b11 = 0.0;
    if (valid) {
        xb = (double)x[3 + 2 * b];
        yb = (double)x[4 + 2 * b];
        b00 = (double)side[b]; b10 = (double)side[(size_t)side_n + b]; b11 = (double)side[(size_t)2 * side_n + b];
    }
    const double gb = 2.0 * gate * (b00 + b11) * FD_SLACK;
    __syncthreads();
    const int lane = tid & 63;
    for (int ai = 0; ai < na; ++ai) {
        const int a = a0 + ai;
        const double dx = xb - s_x[ai], dy = yb - s_y[ai];
        const double r2 = dx * dx + dy * dy;
        const bool surv = valid && a < b && r2 < s_g[ai] + gb;
        if (!__any(surv)) continue;                                      // wave-uniform: survivors are rare
        bool dup = false;
        if (surv) {
            const int fa = 3 + 2 * a, fb = 3 + 2 * b;                    // fb + i > fa + j: the stored triangle holds P_ba
            const double c00 = (double)P[p_off(ld, L, fb, fa)], c10 = (double)P[p_off(ld, L, fb + 1, fa)];
            const double c01 = (double)P[p_off(ld, L, fb, fa + 1)], c11 = (double)P[p_off(ld, L, fb + 1, fa + 1)];
            // P_ab = [c00 c10; c01 c11];  D = ((P_aa + P_bb) - P_ab) - P_ab', then (D + D') / 2
            const double D00 = ((s_00[ai] + b00) - c00) - c00;
            const double D11 = ((s_11[ai] + b11) - c11) - c11;
            const double D01 = ((s_10[ai] + b10) - c10) - c01, D10 = ((s_10[ai] + b10) - c01) - c10;
            const double Ds = (D01 + D10) * 0.5;
            const double det = D00 * D11 - Ds * Ds;
            if (D00 > 0.0 && det > 0.0) dup = (D11 * dx * dx - 2.0 * Ds * dx * dy + D00 * dy * dy) / det < gate;
        }
        const unsigned long long m = __ballot(dup);
        if (m == 0ull) continue;
        const int first = __ffsll((long long)m) - 1;
        unsigned long long base = 0ull;
        if (lane == first) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
        base = __shfl(base, first);
        if (dup) {
            const unsigned long long slot = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
            if (slot < cap) pairs[slot] = make_int2(a + 1, b + 1);       // (unordered: the host sorts the short list)
        }
    }
}

struct MergeArgs {
    int fa[SLAM_MERGE_MAX], fb[SLAM_MERGE_MAX];      // first state index of the survivor / of the landmark that leaves
    double Rc[4];
    int cnt;
};

constexpr int MK = 2 * SLAM_MERGE_MAX;               // 16: the panel's columns, one chunk of the down-date
constexpr int MP = MK + 1;

// column j of P H': P[r, fa_q + c] - P[r, fb_q + c],  q = j / 2, c = j % 2
template <typename T>
__device__ __forceinline__ double merge_pht(const T* __restrict__ P, int ld, int L, const int* fa, const int* fb, int r, int j) {
    const int q = j >> 1, c = j & 1;
    return (double)sym_at(P, ld, L, r, fa[q] + c) - (double)sym_at(P, ld, L, r, fb[q] + c);
}

// the pairs' state indices from the kernel arguments into LDS (constant indices only: a lane-dependent index into the
// argument block would send it through private memory)
__device__ __forceinline__ void merge_tables(const MergeArgs& A, int* fa, int* fb) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int p = 0; p < SLAM_MERGE_MAX; ++p) {
            fa[p] = A.fa[p];
            fb[p] = A.fb[p];
        }
    }
    __syncthreads();
}

// One wave.  S = H P H' + blockdiag(Rc), symmetrised; chol; C = inv(chol(S)) (upper) -> Cout [16][16], g = C C' v -> gout [16].
// Rows / columns >= k are the identity (the existing factorisation pads the same way).  status[0] = 1: S is not positive
// definite, nothing else is written.
template <typename T>
__global__ __launch_bounds__(64) void merge_factor_kernel(const T* __restrict__ x, const T* __restrict__ P, int ld, MergeArgs A,
                                                           double* __restrict__ Cout, double* __restrict__ gout,
                                                           int32_t* __restrict__ status) {
    constexpr int L = kTileLog2<T>;
    __shared__ double M[MK][MP], Li[MK][MP], v[MK], y[MK];
    __shared__ int fa[SLAM_MERGE_MAX], fb[SLAM_MERGE_MAX];
    const int tid = threadIdx.x, k = 2 * A.cnt;
    merge_tables(A, fa, fb);
    const double R00 = A.Rc[0], R10 = A.Rc[1], R01 = A.Rc[2], R11 = A.Rc[3];      // column-major, as the header's R
    for (int e = tid; e < MK * MK; e += 64) {
        const int i = e >> 4, j = e & 15;
        double s = i == j ? 1.0 : 0.0;
        if (i < k && j < k) {
            const int p = i >> 1, r = i & 1;
            s = merge_pht(P, ld, L, fa, fb, fa[p] + r, j) - merge_pht(P, ld, L, fa, fb, fb[p] + r, j);
            if ((j >> 1) == p) s += r ? ((j & 1) ? R11 : R10) : ((j & 1) ? R01 : R00);
        }
        M[i][j] = s;
    }
    if (tid < MK) {
        double d = 0.0;
        if (tid < k) {
            const int p = tid >> 1, r = tid & 1;
            d = -((double)x[fa[p] + r] - (double)x[fb[p] + r]);
        }
        v[tid] = d;
    }
    __syncthreads();
    {   // S = (S + S') / 2: lane i keeps row i of the lower triangle
        double row[MK];
#pragma unroll
        for (int j = 0; j < MK; ++j) row[j] = tid < MK ? (M[tid][j] + M[j][tid]) * 0.5 : 0.0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MK; ++j)
            if (tid < MK) M[tid][j] = row[j];
    }
    __syncthreads();
    // right-looking Cholesky S = L L', lane i owns row i
    bool ok = true;
    for (int j = 0; j < MK; ++j) {
        const double piv = M[j][j];
        if (!(piv > 0.0) || !(piv < INFINITY)) { ok = false; break; }      // (every lane reads the same word: uniform)
        const double d = sqrt(piv);
        __syncthreads();
        if (tid >= j && tid < MK) M[tid][j] = M[tid][j] / d;
        __syncthreads();
        if (tid > j && tid < MK) {
            const double lij = M[tid][j];
            for (int c = j + 1; c <= tid; ++c) M[tid][c] -= lij * M[c][j];
        }
        __syncthreads();
    }
    if (tid == 0) status[0] = ok ? 0 : 1;
    if (!ok) return;
    // inv(L): lane c solves L X[:, c] = e_c
    if (tid < MK) {
        for (int i = 0; i < MK; ++i) {
            double s = i == tid ? 1.0 : 0.0;
            for (int m = tid; m < i; ++m) s -= M[i][m] * Li[m][tid];
            Li[i][tid] = i < tid ? 0.0 : s / M[i][i];
        }
    }
    __syncthreads();
    if (tid < MK) {      // y = C' v = inv(L) v
        double s = 0.0;
        for (int m = 0; m <= tid; ++m) s += Li[tid][m] * v[m];
        y[tid] = s;
    }
    __syncthreads();
    if (tid < MK) {      // g = C y = inv(L)' y
        double s = 0.0;
        for (int m = tid; m < MK; ++m) s += Li[m][tid] * y[m];
        gout[tid] = tid < k ? s : 0.0;
    }
    for (int e = tid; e < MK * MK; e += 64) {       // C[i][j] = inv(L)[j][i], zero outside the leading k x k block
        const int i = e >> 4, j = e & 15;
        Cout[e] = (i < k && j < k && i <= j) ? Li[j][i] : 0.0;
    }
}

// One thread per state row r: PHt[r, :] (k column differences of the symmetric view), W1[r, :] = PHt[r, :] C as the handle's
// dtype, zero-padded to 16 columns, and x[r] += PHt[r, :] g.
template <typename T>
__global__ __launch_bounds__(256) void merge_panel_kernel(T* __restrict__ x, const T* __restrict__ P, int ld, int n, MergeArgs A,
                                                           const double* __restrict__ Cin, const double* __restrict__ gin,
                                                           T* __restrict__ W1, int pitchW, const int32_t* __restrict__ status) {
    constexpr int L = kTileLog2<T>;
    if (status[0] != 0) return;
    __shared__ double Cs[MK * MK], gs[MK];
    __shared__ int fa[SLAM_MERGE_MAX], fb[SLAM_MERGE_MAX];
    merge_tables(A, fa, fb);
    Cs[threadIdx.x] = Cin[threadIdx.x];
    if (threadIdx.x < MK) gs[threadIdx.x] = gin[threadIdx.x];
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int k = 2 * A.cnt;
    double pht[MK];
#pragma unroll
    for (int j = 0; j < MK; ++j) pht[j] = j < k ? merge_pht(P, ld, L, fa, fb, r, j) : 0.0;
    double dxr = 0.0;
    T out[MK];
#pragma unroll
    for (int j = 0; j < MK; ++j) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i <= j; ++i) s += pht[i] * Cs[i * MK + j];
        out[j] = (T)s;
        dxr += pht[j] * gs[j];
    }
    T* __restrict__ w = W1 + (size_t)r * pitchW;
#pragma unroll
    for (int j = 0; j < MK; ++j) w[j] = out[j];
    x[r] = (T)((double)x[r] + dxr);
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

template <typename T>
int find_typed(slam_ekf* h, double gate, std::vector<int2>& found, unsigned long long want, unsigned long long* total) {
    const int N = h->N;
    *total = 0;
    found.clear();
    if (N < 2) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        return SLAM_OK;
    }
    const dim3 grid((N + FD_TB - 1) / FD_TB, (N + FD_TA - 1) / FD_TA);
    // the first `want` pairs in lexicographic order need every pair: a second pass with a larger buffer when the first was short
    unsigned long long cap = want ? std::max<unsigned long long>(want, 4096) : 0;
    for (int pass = 0; pass < 2; ++pass) {
        DevBuf buf;
        HIP_TRY(hipMalloc(&buf.p, 16 + sizeof(int2) * (size_t)cap));
        unsigned long long* cursor = (unsigned long long*)buf.p;
        int2* d_pairs = (int2*)((char*)buf.p + 16);
        HIP_TRY(hipMemsetAsync(cursor, 0, 16, h->stream));
        hipLaunchKernelGGL(find_dup_kernel<T>, grid, dim3(FD_TB), 0, h->stream, (const T*)h->x, (const T*)h->P, h->ld, (const T*)h->Pside,
                           h->npad / 2, N, gate, d_pairs, cap, cursor);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(total, cursor, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (want && *total > cap && pass == 0) {
            cap = *total;
            continue;
        }
        const size_t got = (size_t)std::min<unsigned long long>(*total, cap);
        found.resize(got);
        if (got) HIP_TRY(hipMemcpy(found.data(), d_pairs, sizeof(int2) * got, hipMemcpyDeviceToHost));
        break;
    }
    std::sort(found.begin(), found.end(), [](const int2& p, const int2& q) { return p.x != q.x ? p.x < q.x : p.y < q.y; });
    return SLAM_OK;
}

template <typename T>
int merge_front_typed(slam_ekf* h, const MergeArgs& A) {
    const int n = 3 + 2 * h->N;
    hipLaunchKernelGGL(merge_factor_kernel<T>, dim3(1), dim3(64), 0, h->stream, (const T*)h->x, (const T*)h->P, h->ld, A, h->Cmat,
                       h->gvec, h->d_status);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(merge_panel_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, h->stream, (T*)h->x, (const T*)h->P, h->ld, n, A,
                       (const double*)h->Cmat, (const double*)h->gvec, (T*)h->W1, 2 * h->kcap, (const int32_t*)h->d_status);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

}  // namespace

// pairs_out: min(count, cap) pairs (a, b), a < b, ascending; *count: every duplicate pair of the map.  Synchronises.
int launch_find_duplicates(slam_ekf* h, double gate, int32_t* pairs_out, int cap, int* count) {
    std::vector<int2> found;
    unsigned long long total = 0;
    const int rc = h->dtype == SLAM_F32 ? find_typed<float>(h, gate, found, (unsigned long long)cap, &total)
                                        : find_typed<double>(h, gate, found, (unsigned long long)cap, &total);
    if (rc) return rc;
    *count = total > 0x7fffffffull ? 0x7fffffff : (int)total;
    const size_t give = std::min<size_t>(found.size(), (size_t)cap);
    for (size_t i = 0; i < give; ++i) {
        pairs_out[2 * i] = found[i].x;
        pairs_out[2 * i + 1] = found[i].y;
    }
    return SLAM_OK;
}

// keep[p], gone[p]: 1-based ids, validated by the caller; the update workspace exists (kcap >= 32).  Enqueues the front half and
// the down-date; d_status[0] tells whether S was positive definite (every later stage skips itself when it was not).
int launch_merge_update(slam_ekf* h, const int32_t* keep, const int32_t* gone, int cnt, const double Rc[4]) {
    MergeArgs A;
    memset(&A, 0, sizeof(A));
    A.cnt = cnt;
    for (int p = 0; p < cnt; ++p) {
        A.fa[p] = 3 + 2 * (keep[p] - 1);
        A.fb[p] = 3 + 2 * (gone[p] - 1);
    }
    for (int i = 0; i < 4; ++i) A.Rc[i] = Rc ? Rc[i] : 0.0;
    const int rc = h->dtype == SLAM_F32 ? merge_front_typed<float>(h, A) : merge_front_typed<double>(h, A);
    if (rc) return rc;
    return launch_downdate(h, MK, h->W1, h->W1, 2 * h->kcap, (const int32_t*)nullptr, 0, MK, nullptr);
}
