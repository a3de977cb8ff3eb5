// ekf_local.hip -- compressed local-area updates for the EKF: slam_ekf_local_* (include/ext/slamhip_local.h states the rule, the
// launch chain of close and its bound; tests/local_ref.py runs the rule literally).  libslamhip_local.so.
//
// PER STEP, on the local handle's stream, around the product call on the local handle:
//     local_rows_kernel    predict: phi[0:3, :] <- Gv phi[0:3, :];  augment: the new rows Gxv phi[0:3, :].  The heading is read on
//                          the device BEFORE the product call changes it (one stream).
//     local_pre_kernel     update: E = H phi from the local mean before the update (obs_model of device_math.h, the Jacobian the
//                          update itself forms), a thread per entry.
//     local_post_lds_kernel  update, k <= 128 (see there);  for larger k:
//     local_post_kernel    update: a workgroup per 16 columns J of n0.  Y_J = C' E_J and Z_J = C Y_J go through a global scratch
//                          that only this workgroup reads back (behind its own barriers), then theta_J += E_J' g,
//                          psi[:, J] += E' Z_J, phi[:, J] -= W Y_J with C, g, W from the local handle's update workspace (Cmat,
//                          gvec, W1).  Returns at once when the update's status word is set.  Column blocks are disjoint: every
//                          entry of phi, psi, theta has one writer and E is only read.
// CLOSE, on the global handle's stream (slam_between orders it behind the local stream): gather, T = A0 psi, x_b, the trailing
// product on the matrix cores, A1 = A0 phi', the scatter, the side array.  Operands of the trailing product are K-major
// (column-major n_pad x K): the fragment of k-step kx for the lanes li of a block is one coalesced run, as the tiles of
// ekf_factor.hip's trailing update are.  OWNERSHIP: gather / dense write their own scratch; x_b one thread a row; trail one
// workgroup a tile, one lane an entry (and its mirror inside a diagonal tile); scatter one thread per unordered pair {r, a(i)}.
// No atomics, no LDS beyond the dense kernel's two operand slabs, all offsets 64-bit.
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/slamhip_copy.h"
#include "../../include/ext/slamhip_local.h"
#include "device_math.h"

struct slam_ekf_local {
    slam_ekf* G;                  // the global handle (borrowed)
    slam_ekf* A;                  // the local handle (owned)
    int max_local, pl;            // pl = 3 + 2 max_local: the row pitch of phi, psi, E, Y, Z
    int open, cnt, n0, added, steps, N_open;
    std::vector<int32_t> ids;
    double *phi, *psi, *theta;    // [pl][pl], [pl][pl], [pl]
    double *E, *Ysc, *Zsc;        // [kcap][pl] each
    int kcap;
    int32_t* d_idf;               // [max_local]
    double* d_zn;                 // [2 max_local]
    void* h_stage;                // pinned: the idf / zn of the call in flight
    hipEvent_t stage_ev;
    int stage_pending;
    // close: grow-only scratch
    void *A0, *Tm, *A1;
    size_t a0_bytes, a1_bytes;
    int32_t *d_g2l, *d_l2g;
    int g2l_cap;
};

namespace {

constexpr int GRID_MAX = 2048;
constexpr int JB = 16;            // columns of n0 a workgroup of the post kernel owns

__global__ __launch_bounds__(256) void local_init_kernel(double* __restrict__ phi, double* __restrict__ psi, double* __restrict__ theta,
                                                          int pl, int n0) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= n0) return;
    phi[(size_t)i * pl + j] = i == j ? 1.0 : 0.0;
    psi[(size_t)i * pl + j] = 0.0;
    if (i == 0) theta[j] = 0.0;
}

// predict (nn == 0): rows 0, 1 of phi;  augment: rows na + 2 a, na + 2 a + 1 for the observations a < nn (blockIdx.y)
template <typename T>
__global__ __launch_bounds__(256) void local_rows_kernel(double* __restrict__ phi, int pl, int n0, const T* __restrict__ x, double v,
                                                          double g, double dt, const double* __restrict__ zn, int nn, int na) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n0) return;
    const double p = (double)x[2];
    const double f0 = phi[j], f1 = phi[(size_t)pl + j], f2 = phi[(size_t)2 * pl + j];
    if (nn == 0) {
        const double vts = v * dt * sin(g + p), vtc = v * dt * cos(g + p);
        phi[j] = f0 - vts * f2;
        phi[(size_t)pl + j] = f1 + vtc * f2;
        return;
    }
    const int a = blockIdx.y;
    const double r = zn[2 * a], b = zn[2 * a + 1];
    const double s = sin(p + b), co = cos(p + b);
    phi[(size_t)(na + 2 * a) * pl + j] = f0 - r * s * f2;
    phi[(size_t)(na + 2 * a + 1) * pl + j] = f1 + r * co * f2;
}

template <typename T>
__global__ __launch_bounds__(256) void local_pre_kernel(double* __restrict__ E, const double* __restrict__ phi, int pl, int n0,
                                                         const T* __restrict__ x, const int32_t* __restrict__ idf) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= n0) return;
    const int f = 3 + 2 * (idf[i] - 1);
    const ObsModel om = obs_model((double)x[0], (double)x[1], (double)x[2], (double)x[f], (double)x[f + 1]);
    const double p0 = phi[j], p1 = phi[(size_t)pl + j], p2 = phi[(size_t)2 * pl + j];
    const double q0 = phi[(size_t)f * pl + j], q1 = phi[(size_t)(f + 1) * pl + j];
    E[(size_t)(2 * i) * pl + j] = om.Hv[0] * p0 + om.Hv[1] * p1 + om.Hv[2] * p2 + om.Hf[0] * q0 + om.Hf[1] * q1;
    E[(size_t)(2 * i + 1) * pl + j] = om.Hv[3] * p0 + om.Hv[4] * p1 + om.Hv[5] * p2 + om.Hf[2] * q0 + om.Hf[3] * q1;
}

template <typename T>
__global__ __launch_bounds__(256) void local_post_kernel(double* __restrict__ phi, double* __restrict__ psi, double* __restrict__ theta,
                                                          const double* __restrict__ E, double* Ysc, double* Zsc, int pl, int n0, int na,
                                                          int k, const double* __restrict__ Cm, int cp, const double* __restrict__ gv,
                                                          const T* __restrict__ W, int pw, const int32_t* __restrict__ status) {
    if (status[0] != 0) return;                                           // (uniform: the update did not happen)
    const int tj = threadIdx.x & (JB - 1), tr = threadIdx.x >> 4;
    const int j = blockIdx.x * JB + tj;
    const bool act = j < n0;
    if (act) {
        for (int r = tr; r < k; r += 16) {                                // Y = C' E, C upper
            double s = 0.0;
            for (int i = 0; i <= r; ++i) s += Cm[(size_t)i * cp + r] * E[(size_t)i * pl + j];
            Ysc[(size_t)r * pl + j] = s;
        }
    }
    __syncthreads();
    if (act) {
        for (int i = tr; i < k; i += 16) {                                // Z = C Y
            double s = 0.0;
            for (int r = i; r < k; ++r) s += Cm[(size_t)i * cp + r] * Ysc[(size_t)r * pl + j];
            Zsc[(size_t)i * pl + j] = s;
        }
        if (tr == 0) {
            double s = 0.0;
            for (int i = 0; i < k; ++i) s += E[(size_t)i * pl + j] * gv[i];
            theta[j] += s;
        }
    }
    __syncthreads();
    if (!act) return;
    for (int a = tr; a < n0; a += 16) {                                   // psi[:, J] += E' Z_J
        double s = 0.0;
        for (int i = 0; i < k; ++i) s += E[(size_t)i * pl + a] * Zsc[(size_t)i * pl + j];
        psi[(size_t)a * pl + j] += s;
    }
    for (int r = tr; r < na; r += 16) {                                   // phi[:, J] -= W Y_J
        const T* __restrict__ w = W + (size_t)r * pw;
        double s = 0.0;
        for (int c = 0; c < k; ++c) s += (double)w[c] * Ysc[(size_t)c * pl + j];
        phi[(size_t)r * pl + j] -= s;
    }
}

// The same rules for k <= POST_LDS_K with E_J, Y_J and Z_J in LDS and the rows of psi and phi cut into blocks of POST_ROWS over
// blockIdx.y: every workgroup of a column block forms Y_J and Z_J for itself (k^2 x 16 multiply-adds, no more than its share of
// the rank-k updates), so that nothing passes between workgroups.  The sums run in the order of local_post_kernel.
constexpr int POST_LDS_K = 128, POST_ROWS = 64;

template <typename T>
__global__ __launch_bounds__(256) void local_post_lds_kernel(double* __restrict__ phi, double* __restrict__ psi, double* __restrict__ theta,
                                                              const double* __restrict__ E, int pl, int n0, int na, int k,
                                                              const double* __restrict__ Cm, int cp, const double* __restrict__ gv,
                                                              const T* __restrict__ W, int pw, const int32_t* __restrict__ status) {
    extern __shared__ double post_lds[];
    if (status[0] != 0) return;                                           // (uniform: the update did not happen)
    double* Es = post_lds;
    double* Ys = post_lds + (size_t)k * JB;
    double* Zs = post_lds + (size_t)2 * k * JB;
    const int tj = threadIdx.x & (JB - 1), tr = threadIdx.x >> 4;
    const int j = blockIdx.x * JB + tj;
    const bool act = j < n0;
    for (int r = tr; r < k; r += 16) Es[r * JB + tj] = act ? E[(size_t)r * pl + j] : 0.0;
    __syncthreads();
    for (int r = tr; r < k; r += 16) {                                    // Y = C' E, C upper
        double s = 0.0;
        for (int i = 0; i <= r; ++i) s += Cm[(size_t)i * cp + r] * Es[i * JB + tj];
        Ys[r * JB + tj] = s;
    }
    __syncthreads();
    for (int i = tr; i < k; i += 16) {                                    // Z = C Y
        double s = 0.0;
        for (int r = i; r < k; ++r) s += Cm[(size_t)i * cp + r] * Ys[r * JB + tj];
        Zs[i * JB + tj] = s;
    }
    if (blockIdx.y == 0 && tr == 0 && act) {
        double s = 0.0;
        for (int i = 0; i < k; ++i) s += Es[i * JB + tj] * gv[i];
        theta[j] += s;
    }
    __syncthreads();
    if (!act) return;
    const int r0 = blockIdx.y * POST_ROWS;
    const int a1 = r0 + POST_ROWS < n0 ? r0 + POST_ROWS : n0, r1 = r0 + POST_ROWS < na ? r0 + POST_ROWS : na;
    for (int a = r0 + tr; a < a1; a += 16) {                              // psi[:, J] += E' Z_J
        double s = 0.0;
        for (int i = 0; i < k; ++i) s += E[(size_t)i * pl + a] * Zs[i * JB + tj];
        psi[(size_t)a * pl + j] += s;
    }
    for (int r = r0 + tr; r < r1; r += 16) {                              // phi[:, J] -= W Y_J
        const T* __restrict__ w = W + (size_t)r * pw;
        double s = 0.0;
        for (int c = 0; c < k; ++c) s += (double)w[c] * Ys[c * JB + tj];
        phi[(size_t)r * pl + j] -= s;
    }
}

// ---- close ------------------------------------------------------------------------------------------------------------------------
// A0[k ldA + r] = P[r, l2g[k]] (symmetric view) for r < n, k < n0; zero elsewhere below (ldA, Kp)
template <typename T>
__global__ __launch_bounds__(256) void local_gather_kernel(T* __restrict__ A0, int ldA, const T* __restrict__ P, int ld, int n, int n0,
                                                            const int32_t* __restrict__ l2g) {
    constexpr int L = kTileLog2<T>;
    const int r = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (r >= ldA) return;
    T v = (T)0;
    if (r < n && k < n0) v = sym_at(P, ld, L, r, l2g[k]);
    A0[(size_t)k * ldA + r] = v;
}

// Out[i ldA + r] = (T) sum_j A0[j ldA + r] M[i smi + j smj], one double chain, j ascending; zero for i >= nout, r >= n and the
// rows of A (g2l[r] >= 0)
template <typename T>
__global__ __launch_bounds__(256) void local_dense_kernel(T* __restrict__ Out, const T* __restrict__ A0, int ldA, int n, int K,
                                                           const double* __restrict__ M, long long smi, long long smj, int nout,
                                                           int nout_pad, const int32_t* __restrict__ g2l) {
    __shared__ double As[16][64], Ms[16][65];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int r0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    for (int j0 = 0; j0 < K; j0 += 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = threadIdx.x + 256 * q;
            const int jj = e >> 6, rr = e & 63;
            As[jj][rr] = (j0 + jj < K) ? (double)A0[(size_t)(j0 + jj) * ldA + r0 + rr] : 0.0;
            const int ii = e >> 4, j2 = e & 15;
            Ms[j2][ii] = (i0 + ii < nout && j0 + j2 < K) ? M[(long long)(i0 + ii) * smi + (long long)(j0 + j2) * smj] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            double a[4], m[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = As[jj][tx + 16 * q];
#pragma unroll
            for (int p = 0; p < 4; ++p) m[p] = Ms[jj][ty + 16 * p];
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_fma(a[q], m[p], acc[p][q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = i0 + ty + 16 * p;
        if (i >= nout_pad) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = r0 + tx + 16 * q;
            const bool live = i < nout && r < n && g2l[r] < 0;
            Out[(size_t)i * ldA + r] = live ? (T)acc[p][q] : (T)0;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void local_xb_kernel(T* __restrict__ x, const T* __restrict__ A0, int ldA, int n, int n0,
                                                        const double* __restrict__ theta, const int32_t* __restrict__ g2l) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n || g2l[r] >= 0) return;
    double s = 0.0;
    for (int j = 0; j < n0; ++j) s = __builtin_fma((double)A0[(size_t)j * ldA + r], theta[j], s);
    if (s != 0.0) x[r] = (T)((double)x[r] + s);
}

// P[r, c] -= sum_k Tm[r, k] A0[c, k] over the tiles (I, J), J <= I < Tw
template <typename T>
__global__ __launch_bounds__(256) void local_trail_kernel(T* __restrict__ P, int ld, const T* __restrict__ Tm, const T* __restrict__ A0,
                                                           int ldA, int Kp, int Tw, long long items) {
    typedef MfmaTile<T> H;
    constexpr int L = H::L, E = 1 << L, MB = H::MB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & (MB - 1), half = lane >> H::LSH;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        int I, J;
        tile_of(w, Tw, &I, &J);
        if (I == J && wc > wr) continue;                                 // the strict upper quadrant: written as the mirror of the lower
        typename H::Acc acc[2][2];                                       // [column block][row block]
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int g = 0; g < H::NREG; ++g) acc[cb][rb][g] = (T)0;
        const T* __restrict__ YJ = A0 + ((size_t)J << L) + 2 * MB * wc + li;
        const T* __restrict__ XI = Tm + ((size_t)I << L) + 2 * MB * wr + li;
        for (int kk = 0; kk < Kp / H::KS; ++kk) {
            const size_t kx = (size_t)(kk * H::KS + half) * ldA;
            T a[2], b[2];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) a[cb] = YJ[kx + MB * cb];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) b[rb] = XI[kx + MB * rb];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) acc[cb][rb] = H::mfma(a[cb], b[rb], acc[cb][rb]);
        }
        T* tgt = P + tile_base(I, J, ld >> L, L);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int g = 0; g < H::NREG; ++g) {
                    const int col = 2 * MB * wc + MB * cb + H::out_i(g, half);
                    const int row = 2 * MB * wr + MB * rb + li;
                    if (I == J) {
                        if (row < col) continue;
                        const T v = tgt[col * E + row] - acc[cb][rb][g];
                        tgt[col * E + row] = v;
                        if (row != col) tgt[row * E + col] = v;
                    } else {
                        tgt[col * E + row] -= acc[cb][rb][g];
                    }
                }
    }
}

// entry {r, l2g[ci]} of the new global matrix, r < nn (new global size), ci < na: rows of A from the local state, rows of B from A1
template <typename T>
__global__ __launch_bounds__(256) void local_scatter_kernel(T* __restrict__ x, T* __restrict__ P, int ld, int nn, int na,
                                                             const T* __restrict__ xl, const T* __restrict__ Pl, int ldl,
                                                             const T* __restrict__ A1, int ldA, const int32_t* __restrict__ g2l,
                                                             const int32_t* __restrict__ l2g) {
    constexpr int L = kTileLog2<T>;
    const int r = blockIdx.x * 256 + threadIdx.x, ci = blockIdx.y;
    if (r >= nn) return;
    const int li = g2l[r], gc = l2g[ci];
    T v;
    if (li >= 0) {
        if (li < ci) return;                                              // the pair's other thread writes both positions
        v = Pl[p_off(ldl, L, li, ci)];
        if (ci == 0) x[r] = xl[li];
    } else {
        v = A1[(size_t)ci * ldA + r];
    }
    p_store_sym(P, ld, L, r, gc, v);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int ensure_k(slam_ekf_local* L, int k) {
    if (k <= L->kcap) return SLAM_OK;
    const int kc = round_up(k, 64);
    HIP_TRY(hipStreamSynchronize(L->A->stream));
    if (L->E) (void)hipFree(L->E);
    if (L->Ysc) (void)hipFree(L->Ysc);
    if (L->Zsc) (void)hipFree(L->Zsc);
    L->E = L->Ysc = L->Zsc = nullptr;
    L->kcap = 0;
    const size_t bytes = sizeof(double) * (size_t)kc * L->pl;
    HIP_TRY(hipMalloc((void**)&L->E, bytes));
    HIP_TRY(hipMalloc((void**)&L->Ysc, bytes));
    HIP_TRY(hipMalloc((void**)&L->Zsc, bytes));
    L->kcap = kc;
    return SLAM_OK;
}

// src -> dst (device) through the pinned staging buffer, on the local stream
int stage(slam_ekf_local* L, void* dst, const void* src, size_t bytes) {
    if (L->stage_pending) {
        HIP_TRY(hipEventSynchronize(L->stage_ev));
        L->stage_pending = 0;
    }
    memcpy(L->h_stage, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, L->h_stage, bytes, hipMemcpyHostToDevice, L->A->stream));
    HIP_TRY(hipEventRecord(L->stage_ev, L->A->stream));
    L->stage_pending = 1;
    return SLAM_OK;
}

int check_open(slam_ekf_local* L) {
    ARG_CHECK(L != nullptr, "null handle");
    ARG_CHECK(L->open, "no area is open");
    return SLAM_OK;
}

template <typename T>
int close_typed(slam_ekf_local* L, int na, int n_old, int n_new) {
    constexpr int Lg = kTileLog2<T>;
    slam_ekf* G = L->G;
    slam_ekf* A = L->A;
    const int n0 = L->n0, Kp = round_up(n0, 16), ldA = G->npad;
    hipStream_t s = G->stream;
    T *A0 = (T*)L->A0, *Tm = (T*)L->Tm, *A1 = (T*)L->A1;
    const dim3 rows((ldA + 255) / 256);
    hipLaunchKernelGGL(local_gather_kernel<T>, dim3(rows.x, Kp), dim3(256), 0, s, A0, ldA, (const T*)G->P, G->ld, n_old, n0,
                       (const int32_t*)L->d_l2g);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(local_dense_kernel<T>, dim3(ldA / 64, (Kp + 63) / 64), dim3(256), 0, s, Tm, (const T*)A0, ldA, n_old, n0,
                       (const double*)L->psi, 1LL, (long long)L->pl, n0, Kp, (const int32_t*)L->d_g2l);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(local_xb_kernel<T>, dim3((n_old + 255) / 256), dim3(256), 0, s, (T*)G->x, (const T*)A0, ldA, n_old, n0,
                       (const double*)L->theta, (const int32_t*)L->d_g2l);
    HIP_TRY(hipGetLastError());
    const int Tw = (n_old + (1 << Lg) - 1) >> Lg;
    const long long items = (long long)Tw * (Tw + 1) / 2;
    hipLaunchKernelGGL(local_trail_kernel<T>, dim3((unsigned)(items < GRID_MAX ? items : GRID_MAX)), dim3(256), 0, s, (T*)G->P, G->ld,
                       (const T*)Tm, (const T*)A0, ldA, Kp, Tw, items);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(local_dense_kernel<T>, dim3(ldA / 64, (na + 63) / 64), dim3(256), 0, s, A1, (const T*)A0, ldA, n_old, n0,
                       (const double*)L->phi, (long long)L->pl, 1LL, na, na, (const int32_t*)L->d_g2l);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(local_scatter_kernel<T>, dim3((n_new + 255) / 256, na), dim3(256), 0, s, (T*)G->x, (T*)G->P, G->ld, n_new, na,
                       (const T*)A->x, (const T*)A->P, A->ld, (const T*)A1, ldA, (const int32_t*)L->d_g2l, (const int32_t*)L->d_l2g);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

int ensure_close_scratch(slam_ekf_local* L, int na, int n_new) {
    slam_ekf* G = L->G;
    const size_t ldA = (size_t)G->npad;
    const size_t a0 = G->esz * ldA * (size_t)round_up(L->n0, 64), a1 = G->esz * ldA * (size_t)round_up(na, 64);
    if (a0 > L->a0_bytes) {
        if (L->A0) (void)hipFree(L->A0);
        if (L->Tm) (void)hipFree(L->Tm);
        L->A0 = L->Tm = nullptr;
        L->a0_bytes = 0;
        HIP_TRY(hipMalloc(&L->A0, a0));
        HIP_TRY(hipMalloc(&L->Tm, a0));
        L->a0_bytes = a0;
    }
    if (a1 > L->a1_bytes) {
        if (L->A1) (void)hipFree(L->A1);
        L->A1 = nullptr;
        L->a1_bytes = 0;
        HIP_TRY(hipMalloc(&L->A1, a1));
        L->a1_bytes = a1;
    }
    if (G->npad > L->g2l_cap) {
        if (L->d_g2l) (void)hipFree(L->d_g2l);
        L->d_g2l = nullptr;
        L->g2l_cap = 0;
        HIP_TRY(hipMalloc((void**)&L->d_g2l, sizeof(int32_t) * (size_t)G->npad));
        L->g2l_cap = G->npad;
    }
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_ekf_local_create(slam_ekf_local_t* out, slam_ekf_t global, int max_local) {
    SLAM_RANGE();
    ARG_CHECK(out != nullptr, "null argument");
    *out = nullptr;
    ARG_CHECK(global != nullptr, "null handle");
    ARG_CHECK(max_local >= 1 && max_local <= SLAM_LOCAL_MAXLM, "max_local outside 1 .. SLAM_LOCAL_MAXLM");
    HIP_TRY(hipSetDevice(global->device));
    slam_ekf_local* L = new slam_ekf_local();
    L->G = global;
    L->max_local = max_local;
    L->pl = 3 + 2 * max_local;
    int rc = slam_ekf_create(&L->A, global->dtype, max_local, global->device);
    if (rc) {
        delete L;
        return rc;
    }
    const size_t sq = sizeof(double) * (size_t)L->pl * L->pl;
    const size_t stage_bytes = sizeof(double) * 2 * (size_t)max_local;
    hipError_t e = hipMalloc((void**)&L->phi, sq);
    if (e == hipSuccess) e = hipMalloc((void**)&L->psi, sq);
    if (e == hipSuccess) e = hipMalloc((void**)&L->theta, sizeof(double) * (size_t)L->pl);
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_idf, sizeof(int32_t) * (size_t)max_local);
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_zn, stage_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&L->d_l2g, sizeof(int32_t) * (size_t)L->pl);
    if (e == hipSuccess) e = hipHostMalloc(&L->h_stage, stage_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L->stage_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        slam_set_error("local create: %s", hipGetErrorString(e));
        (void)slam_ekf_local_destroy(L);
        return e == hipErrorOutOfMemory ? SLAM_E_NOMEM : SLAM_E_HIP;
    }
    *out = L;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_destroy(slam_ekf_local_t L) {
    if (!L) return SLAM_OK;
    if (L->A) {
        (void)hipSetDevice(L->A->device);
        (void)hipStreamSynchronize(L->A->stream);
        (void)slam_ekf_destroy(L->A);
    }
    void* dev[] = {L->phi, L->psi, L->theta, L->E, L->Ysc, L->Zsc, L->d_idf, L->d_zn, L->A0, L->Tm, L->A1, L->d_g2l, L->d_l2g};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (L->h_stage) (void)hipHostFree(L->h_stage);
    if (L->stage_ev) (void)hipEventDestroy(L->stage_ev);
    delete L;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_open(slam_ekf_local_t L, const int32_t* ids, int cnt) {
    SLAM_RANGE();
    ARG_CHECK(L != nullptr, "null handle");
    ARG_CHECK(!L->open, "an area is already open");
    ARG_CHECK(cnt >= 0 && cnt <= L->max_local, "cnt outside 0 .. max_local");
    ARG_CHECK(cnt == 0 || ids != nullptr, "ids is null");
    int rc = slam_ekf_select(L->A, L->G, ids, cnt);                        // ids out of range or twice: its SLAM_E_BADARG
    if (rc) return rc;
    HIP_TRY(hipSetDevice(L->A->device));
    L->ids.assign(ids, ids + cnt);
    L->cnt = cnt;
    L->n0 = 3 + 2 * cnt;
    L->added = 0;
    L->steps = 0;
    L->N_open = L->G->N;
    hipLaunchKernelGGL(local_init_kernel, dim3((L->n0 + 255) / 256, L->n0), dim3(256), 0, L->A->stream, L->phi, L->psi, L->theta, L->pl,
                       L->n0);
    HIP_TRY(hipGetLastError());
    L->open = 1;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_state(slam_ekf_local_t L, slam_ekf_t* local) {
    ARG_CHECK(L != nullptr && local != nullptr, "null argument");
    *local = L->A;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_predict(slam_ekf_local_t L, double v, double g, double wheelbase, const double* Q, double dt) {
    SLAM_RANGE();
    int rc;
    if ((rc = check_open(L))) return rc;
    ARG_CHECK(Q != nullptr, "null argument");
    slam_ekf* A = L->A;
    HIP_TRY(hipSetDevice(A->device));
    const dim3 grid((L->n0 + 255) / 256);
    if (A->dtype == SLAM_F32)
        hipLaunchKernelGGL(local_rows_kernel<float>, grid, dim3(256), 0, A->stream, L->phi, L->pl, L->n0, (const float*)A->x, v, g, dt,
                           (const double*)nullptr, 0, 0);
    else
        hipLaunchKernelGGL(local_rows_kernel<double>, grid, dim3(256), 0, A->stream, L->phi, L->pl, L->n0, (const double*)A->x, v, g, dt,
                           (const double*)nullptr, 0, 0);
    HIP_TRY(hipGetLastError());
    L->steps++;
    return slam_ekf_predict(A, v, g, wheelbase, Q, dt);
}

extern "C" int slam_ekf_local_update(slam_ekf_local_t L, const double* z, const int32_t* idf_local, int m, const double* R, int form) {
    SLAM_RANGE();
    int rc;
    if ((rc = check_open(L))) return rc;
    ARG_CHECK(form == SLAM_FORM_CHOLESKY, "only SLAM_FORM_CHOLESKY inside a local area");
    ARG_CHECK(m >= 0, "m < 0");
    if (m == 0) return SLAM_OK;
    ARG_CHECK(z != nullptr && idf_local != nullptr && R != nullptr, "null argument");
    slam_ekf* A = L->A;
    ARG_CHECK(m <= L->max_local, "more observations than max_local");
    for (int i = 0; i < m; ++i) ARG_CHECK(idf_local[i] >= 1 && idf_local[i] <= A->N, "local id outside 1 .. the local landmark count");
    HIP_TRY(hipSetDevice(A->device));
    const int k = 2 * m, na = 3 + 2 * A->N;
    if ((rc = ensure_k(L, k))) return rc;
    if ((rc = stage(L, L->d_idf, idf_local, sizeof(int32_t) * (size_t)m))) return rc;
    const dim3 grid((L->n0 + 255) / 256, m);
    if (A->dtype == SLAM_F32)
        hipLaunchKernelGGL(local_pre_kernel<float>, grid, dim3(256), 0, A->stream, L->E, (const double*)L->phi, L->pl, L->n0,
                           (const float*)A->x, (const int32_t*)L->d_idf);
    else
        hipLaunchKernelGGL(local_pre_kernel<double>, grid, dim3(256), 0, A->stream, L->E, (const double*)L->phi, L->pl, L->n0,
                           (const double*)A->x, (const int32_t*)L->d_idf);
    HIP_TRY(hipGetLastError());
    const int urc = slam_ekf_update(A, z, idf_local, m, R, form);
    if (urc != SLAM_OK && urc != SLAM_E_NOTPD) return urc;                // (decided before the update was enqueued, or the runtime failed)
    // the accumulators follow the update on the device: the launch returns at once on the status word of a failed factorisation
    const dim3 pgrid((L->n0 + JB - 1) / JB);
    const dim3 lgrid(pgrid.x, ((na > L->n0 ? na : L->n0) + POST_ROWS - 1) / POST_ROWS);
    const size_t lds = sizeof(double) * 3 * (size_t)k * JB;
    const bool small = k <= POST_LDS_K;
    if (A->dtype == SLAM_F32 && small)
        hipLaunchKernelGGL(local_post_lds_kernel<float>, lgrid, dim3(256), lds, A->stream, L->phi, L->psi, L->theta, (const double*)L->E,
                           L->pl, L->n0, na, k, (const double*)A->Cmat, A->kcap, (const double*)A->gvec, (const float*)A->W1, 2 * A->kcap,
                           (const int32_t*)A->d_status);
    else if (small)
        hipLaunchKernelGGL(local_post_lds_kernel<double>, lgrid, dim3(256), lds, A->stream, L->phi, L->psi, L->theta, (const double*)L->E,
                           L->pl, L->n0, na, k, (const double*)A->Cmat, A->kcap, (const double*)A->gvec, (const double*)A->W1, 2 * A->kcap,
                           (const int32_t*)A->d_status);
    else if (A->dtype == SLAM_F32)
        hipLaunchKernelGGL(local_post_kernel<float>, pgrid, dim3(256), 0, A->stream, L->phi, L->psi, L->theta, (const double*)L->E, L->Ysc,
                           L->Zsc, L->pl, L->n0, na, k, (const double*)A->Cmat, A->kcap, (const double*)A->gvec, (const float*)A->W1,
                           2 * A->kcap, (const int32_t*)A->d_status);
    else
        hipLaunchKernelGGL(local_post_kernel<double>, pgrid, dim3(256), 0, A->stream, L->phi, L->psi, L->theta, (const double*)L->E, L->Ysc,
                           L->Zsc, L->pl, L->n0, na, k, (const double*)A->Cmat, A->kcap, (const double*)A->gvec, (const double*)A->W1,
                           2 * A->kcap, (const int32_t*)A->d_status);
    HIP_TRY(hipGetLastError());
    L->steps++;
    return urc;
}

extern "C" int slam_ekf_local_augment(slam_ekf_local_t L, const double* zn, int nn, const double* R) {
    SLAM_RANGE();
    int rc;
    if ((rc = check_open(L))) return rc;
    ARG_CHECK(nn >= 0, "nn < 0");
    if (nn == 0) return SLAM_OK;
    ARG_CHECK(zn != nullptr && R != nullptr, "null argument");
    slam_ekf* A = L->A;
    if (A->N + nn > L->max_local) {
        slam_set_error("local augment: %d + %d landmarks exceed max_local %d", A->N, nn, L->max_local);
        return SLAM_E_CAPACITY;
    }
    if (L->N_open + L->added + nn > L->G->maxN) {
        slam_set_error("local augment: %d + %d + %d landmarks exceed the global capacity %d", L->N_open, L->added, nn, L->G->maxN);
        return SLAM_E_CAPACITY;
    }
    HIP_TRY(hipSetDevice(A->device));
    if ((rc = stage(L, L->d_zn, zn, sizeof(double) * 2 * (size_t)nn))) return rc;
    const int na = 3 + 2 * A->N;
    const dim3 grid((L->n0 + 255) / 256, nn);
    if (A->dtype == SLAM_F32)
        hipLaunchKernelGGL(local_rows_kernel<float>, grid, dim3(256), 0, A->stream, L->phi, L->pl, L->n0, (const float*)A->x, 0.0, 0.0, 0.0,
                           (const double*)L->d_zn, nn, na);
    else
        hipLaunchKernelGGL(local_rows_kernel<double>, grid, dim3(256), 0, A->stream, L->phi, L->pl, L->n0, (const double*)A->x, 0.0, 0.0, 0.0,
                           (const double*)L->d_zn, nn, na);
    HIP_TRY(hipGetLastError());
    if ((rc = slam_ekf_augment(A, zn, nn, R))) return rc;
    L->added += nn;
    L->steps++;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_close(slam_ekf_local_t L, int* first_new) {
    SLAM_RANGE();
    int rc;
    if ((rc = check_open(L))) return rc;
    slam_ekf* G = L->G;
    slam_ekf* A = L->A;
    ARG_CHECK(G->N == L->N_open, "the global state's N changed while the area was open");
    if (A->pending_status && (rc = slam_ekf_sync(A))) return rc;
    if (G->pending_status && (rc = slam_ekf_sync(G))) return rc;
    HIP_TRY(hipSetDevice(G->device));
    const int na = 3 + 2 * A->N, n_old = 3 + 2 * L->N_open, n_new = n_old + 2 * L->added;
    if ((rc = ensure_close_scratch(L, na, n_new))) return rc;
    std::vector<int32_t> g2l((size_t)G->npad, -1), l2g((size_t)na);
    for (int i = 0; i < na; ++i) {
        const int lm = (i - 3) >> 1, o = (i - 3) & 1;                    // (i >= 3)
        const int g = i < 3 ? i : (lm < L->cnt ? 3 + 2 * (L->ids[lm] - 1) + o : n_old + 2 * (lm - L->cnt) + o);
        l2g[i] = g;
        g2l[g] = i;
    }
    rc = slam_between(G->stream, A->stream, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(L->d_g2l, g2l.data(), sizeof(int32_t) * g2l.size(), hipMemcpyHostToDevice, G->stream));
        HIP_TRY(hipMemcpyAsync(L->d_l2g, l2g.data(), sizeof(int32_t) * l2g.size(), hipMemcpyHostToDevice, G->stream));
        const int rcc = G->dtype == SLAM_F32 ? close_typed<float>(L, na, n_old, n_new) : close_typed<double>(L, na, n_old, n_new);
        if (rcc) return rcc;
        G->N = L->N_open + L->added;
        G->grid_force = 1;                                                // the means moved
        G->pmax_valid = 0;                                                // appended landmarks, rewritten variances
        return launch_side_rebuild(G);
    });
    const hipError_t e = hipStreamSynchronize(G->stream);                 // (also: the host index maps outlive their copies)
    L->open = 0;
    if (rc) return rc;
    HIP_TRY(e);
    if (first_new) *first_new = L->N_open + 1;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_abort(slam_ekf_local_t L) {
    int rc;
    if ((rc = check_open(L))) return rc;
    L->open = 0;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_info(slam_ekf_local_t L, int64_t* out) {
    ARG_CHECK(L != nullptr && out != nullptr, "null argument");
    out[0] = L->open;
    out[1] = L->n0;
    out[2] = L->open || L->n0 ? 3 + 2 * L->A->N : 0;
    out[3] = L->added;
    out[4] = L->steps;
    out[5] = L->N_open;
    out[6] = L->max_local;
    out[7] = 0;
    return SLAM_OK;
}

extern "C" int slam_ekf_local_get(slam_ekf_local_t L, double* phi, double* psi, double* theta) {
    int rc;
    if ((rc = check_open(L))) return rc;
    slam_ekf* A = L->A;
    HIP_TRY(hipSetDevice(A->device));
    HIP_TRY(hipStreamSynchronize(A->stream));
    const int na = 3 + 2 * A->N, n0 = L->n0;
    const size_t row = sizeof(double) * (size_t)n0, pitch = sizeof(double) * (size_t)L->pl;
    if (phi) HIP_TRY(hipMemcpy2D(phi, row, L->phi, pitch, row, (size_t)na, hipMemcpyDeviceToHost));
    if (psi) HIP_TRY(hipMemcpy2D(psi, row, L->psi, pitch, row, (size_t)n0, hipMemcpyDeviceToHost));
    if (theta) HIP_TRY(hipMemcpy(theta, L->theta, row, hipMemcpyDeviceToHost));
    return SLAM_OK;
}
