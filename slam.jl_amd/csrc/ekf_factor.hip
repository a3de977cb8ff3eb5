// ekf_factor.hip -- the Cholesky factor of an EKF state's covariance on the device: slam_ekf_factor_* (include/ext/slamhip_factor.h
// states the rule; tests/factor_ref.py runs it literally).  libslamhip_factor.so.
//
//     P[0 : n, 0 : n] = L L'      a blocked right-looking Cholesky over the tile grid of the state's own layout (device_math.h)
//
// A panel is `pt` tile columns [k0, k0 + w).  For k = k0 .. k0 + w - 1:
//     factor_diag_kernel    (one workgroup)             tile (k, k) -> L_kk in LDS, column by column; pivot statistics
//     factor_panel_kernel   (tiles I > k)               L_Ik = A_Ik L_kk^-T by substitution, a thread per row, L_kk in LDS
//     factor_trail_kernel   (source [k, k + 1))         the targets (I, J), k < J < k0 + w, I >= J: the rest of the panel
// then  factor_trail_kernel (source [k0, k0 + w))       the targets (I, J), J >= k0 + w, I >= J: everything to the right
// OWNERSHIP.  A launch of diag writes tile (k, k) and the status block's entries of tile k; a launch of panel writes the tiles
// (I, k), I > k, each by one workgroup, a row by one thread; a launch of trail writes its target tiles, each by one workgroup, each
// entry by one lane, and READS only tiles of columns < J0 (finished factor tiles, written by earlier launches).  No tile is read
// and written by different workgroups of one launch, so every dependency is a launch boundary: no ready words, no spinning, no
// claim counters.  The grids stride over their tile lists (at most 2048 workgroups).  When a pivot fails, stat[0] is set and
// every later launch returns at once.  No atomics, no private scratch, all offsets 64-bit.
//
// The trailing update runs on the matrix cores in the factor's own precision (no bf16 split: the bound of the header rests on
// one rounding of unit roundoff u per operation).  A tile is column-major, so the fragment of k-step kx -- L[row0 + li, kx] for the
// lanes li of a block -- is one coalesced run of the tile's column kx: the operands go from global memory (the caches) straight
// into the MFMA, wave (wr, wc) of four owning a quadrant as 2 x 2 blocks of 32 x 32 (fp32) / 16 x 16 (fp64).  The A operand
// takes the COLUMN tile (J, p), B the ROW tile (I, p), so a lane of the result holds one row of the target and the read-modify-write
// runs along the tile's columns.
//
// solve / multiply: the same walk over tile columns with two kernels per step (header), L read in its dtype, fp64 arithmetic.
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/ext/slamhip_factor.h"
#include "device_math.h"

struct slam_ekf_factor {
    int dtype, device, maxN;
    int L, E, Tf;                 // tile edge 2^L, tile rows of the allocation
    int pt;                       // panel_tiles in use
    size_t esz;
    void* F;                      // the factor: Tf (Tf + 1) / 2 tiles
    double* xd;                   // [3 + 2 maxN]  x of the last compute, as doubles
    double* stat;                 // [8 + 3 Tf]    [0] failed  [1] index  [2] pivot;  per tile k: [8 + 3 k ..] min l, max l, sum log l
    double* dB;                   // [Tf E][64]    solve: B -> Y in place;  multiply: out
    double* dZ;                   // [Tf E][64]    multiply: Z
    hipStream_t stream;
    std::vector<double> hx, hstat;
    int n, valid;
    double info[8];
};

namespace {

constexpr int GRID_MAX = 2048;
constexpr int DIAG_THREADS = 512;
constexpr int RHS_MAX = 64;
constexpr int SOL_THREADS = 1024;

// the MFMA tile (device_math.h) and CB: the columns the panel's triangular solve holds in registers at a time
template <typename T> struct Fx : MfmaTile<T> {
    static constexpr int CB = sizeof(T) == 4 ? 32 : 16;
};

// ---- copy-in: F <- P[0 : n, 0 : n] of the source, every entry of the tiles below Tn (zero outside n) ---------------------------
// Entry by entry through p_off on both sides (gather_tiles_kernel of ekf_copy.hip), so the two tile edges may differ; the value
// of (r, c) is the one STORED for (max, min).  S -> T is float -> float, double -> double or float -> double: exact.
template <typename T, typename S>
__global__ __launch_bounds__(256) void factor_copyin_kernel(T* __restrict__ F, int Tf, const S* __restrict__ Ps, int lds, int n, int Tn,
                                                             long long items) {
    constexpr int L = Fx<T>::L, E = 1 << L;
    constexpr int LS = Fx<S>::L;
    for (long long q = blockIdx.x; q < items; q += gridDim.x) {
        int I, J;
        tile_of(q, Tn, &I, &J);
        T* __restrict__ tile = F + tile_base(I, J, Tf, L);
        for (int e = threadIdx.x; e < E * E; e += 256) {
            const int r = (I << L) + (e & (E - 1)), c = (J << L) + (e >> L);
            T v = (T)0;
            if (r < n && c < n) {
                const int hi = r > c ? r : c, lo = r > c ? c : r;
                v = (T)Ps[p_off(lds, LS, hi, lo)];
            }
            tile[e] = v;
        }
    }
}

template <typename S>
__global__ __launch_bounds__(256) void factor_x_kernel(double* __restrict__ xd, const S* __restrict__ xs, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) xd[i] = (double)xs[i];
}

// ---- diag: tile (k, k) -> L_kk ------------------------------------------------------------------------------------------------
// Right-looking inside the tile: column j is scaled by 1 / l_jj (a division), then the lower triangle to its right is updated.
// Every thread reads the same pivot from LDS, so the decision to stop is uniform.  The diagonal keeps d_j in LDS until the tile is
// written (l_jj = sqrt(d_j) is recomputed there: the same value).  The strict upper triangle is written as +0.0.
template <typename T>
__global__ __launch_bounds__(DIAG_THREADS) void factor_diag_kernel(T* __restrict__ F, int Tf, int k, int n, double* __restrict__ stat) {
    constexpr int L = Fx<T>::L, E = 1 << L;
    __shared__ T sA[E * E];
    if (stat[0] != 0.0) return;
    T* __restrict__ tile = F + tile_base(k, k, Tf, L);
    const int t = threadIdx.x;
    for (int e = t; e < E * E; e += DIAG_THREADS) sA[e] = tile[e];
    __syncthreads();
    const int m = n - (k << L) < E ? n - (k << L) : E;
    const int rl = t & (E - 1), c_sub = t >> L;
    constexpr int CSTEP = DIAG_THREADS >> L;
    double lsum = 0.0;
    T lmin = (T)INFINITY, lmax = (T)0;
    bool failed = false;
    for (int j = 0; j < m; ++j) {
        const T d = sA[j * E + j];
        if (!(d > (T)0) || isinf(d)) {                                  // (NaN fails the first test)
            if (t == 0) {
                stat[1] = (double)((k << L) + j);
                stat[2] = (double)d;
                stat[0] = 1.0;
            }
            failed = true;
            break;
        }
        const T l = sqrt(d);
        lsum += log((double)l);
        lmin = l < lmin ? l : lmin;
        lmax = l > lmax ? l : lmax;
        for (int r = j + 1 + t; r < m; r += DIAG_THREADS) sA[j * E + r] = sA[j * E + r] / l;
        __syncthreads();
        if (rl < m) {
            const T lr = sA[j * E + rl];
            int c = j + 1 + c_sub;
            for (; c + 3 * CSTEP <= rl; c += 4 * CSTEP) {                 // four independent entries at a time: loads, then stores
                T a[4], b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    a[q] = sA[(c + q * CSTEP) * E + rl];
                    b[q] = sA[j * E + c + q * CSTEP];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) sA[(c + q * CSTEP) * E + rl] = a[q] - lr * b[q];
            }
            for (; c <= rl; c += CSTEP) sA[c * E + rl] -= lr * sA[j * E + c];
        }
        __syncthreads();
    }
    if (failed) return;
    for (int e = t; e < E * E; e += DIAG_THREADS) {
        const int r = e & (E - 1), c = e >> L;
        T v = sA[e];
        if (r == c && c < m) v = sqrt(v);
        if (r < c) v = (T)0;
        tile[e] = v;
    }
    if (t == 0) {
        stat[8 + 3 * k] = (double)lmin;
        stat[8 + 3 * k + 1] = (double)lmax;
        stat[8 + 3 * k + 2] = lsum;
    }
}

// ---- panel: L_Ik = A_Ik L_kk^-T for the tiles I > k ----------------------------------------------------------------------------
// x L_kk' = a for every row a of the tile: x_c = (a_c - sum_{j < c} x_j l_cj) / l_cc.  Thread r owns row r: its accesses
// tile[j E + r] are coalesced over the workgroup, and it reads back only what it stored itself.  Columns go in blocks of CB held in
// registers: the finished columns' contributions first (a runtime loop over j, the block's l_cj one LDS run), then the block's own
// triangle (unrolled).
template <typename T>
__global__ __launch_bounds__(1 << Fx<T>::L) void factor_panel_kernel(T* F, int Tf, int k, int Tn, const double* __restrict__ stat) {
    constexpr int L = Fx<T>::L, E = 1 << L, CB = Fx<T>::CB;
    __shared__ T sL[E * E];
    if (stat[0] != 0.0) return;
    const int r = threadIdx.x;
    {
        const T* __restrict__ lkk = F + tile_base(k, k, Tf, L);
        for (int e = r; e < E * E; e += E) sL[e] = lkk[e];
    }
    __syncthreads();
    for (int I = k + 1 + (int)blockIdx.x; I < Tn; I += gridDim.x) {
        T* tile = F + tile_base(I, k, Tf, L);
        for (int c0 = 0; c0 < E; c0 += CB) {
            T a[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c) a[c] = tile[(size_t)(c0 + c) * E + r];
#pragma unroll 4
            for (int j = 0; j < c0; ++j) {
                const T xj = tile[(size_t)j * E + r];
#pragma unroll
                for (int c = 0; c < CB; ++c) a[c] -= xj * sL[j * E + c0 + c];
            }
#pragma unroll
            for (int c = 0; c < CB; ++c) {
#pragma unroll
                for (int j = 0; j < c; ++j) a[c] -= a[j] * sL[(c0 + j) * E + c0 + c];
                a[c] = a[c] / sL[(c0 + c) * E + c0 + c];
            }
#pragma unroll
            for (int c = 0; c < CB; ++c) tile[(size_t)(c0 + c) * E + r] = a[c];
        }
    }
}

// ---- trail: A_IJ -= sum_{p0 <= p < p1} L_Ip L_Jp' for the targets J0 <= J < J1, J <= I < Tn ----------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void factor_trail_kernel(T* F, int Tf, int Tn, int p0, int p1, int J0, int J1, long long items,
                                                            const double* __restrict__ stat) {
    typedef Fx<T> H;
    constexpr int L = H::L, E = 1 << L, MB = H::MB;
    if (stat[0] != 0.0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & (MB - 1), half = lane >> H::LSH;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        int J = J0;
        long long q = w;
        while (q >= Tn - J) { q -= Tn - J; ++J; }
        const int I = J + (int)q;
        if (I == J && wc > wr) continue;                                 // the strict upper quadrant of a diagonal target: not meaningful
        typename H::Acc acc[2][2];                                       // [column block][row block]
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int g = 0; g < H::NREG; ++g) acc[cb][rb][g] = (T)0;
        for (int p = p0; p < p1; ++p) {
            const T* __restrict__ LJ = F + tile_base(J, p, Tf, L) + 2 * MB * wc + li;
            const T* __restrict__ LI = F + tile_base(I, p, Tf, L) + 2 * MB * wr + li;
#pragma unroll 8
            for (int kk = 0; kk < E / H::KS; ++kk) {
                const int kx = kk * H::KS + half;
                T a[2], b[2];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) a[cb] = LJ[kx * E + MB * cb];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) b[rb] = LI[kx * E + MB * rb];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) acc[cb][rb] = H::mfma(a[cb], b[rb], acc[cb][rb]);
            }
        }
        T* tgt = F + tile_base(I, J, Tf, L);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int g = 0; g < H::NREG; ++g) {
                    const int col = 2 * MB * wc + MB * cb + H::out_i(g, half);
                    const int row = 2 * MB * wr + MB * rb + li;
                    tgt[col * E + row] -= acc[cb][rb][g];
                }
    }
}

// ---- get: a dense block of L ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void factor_get_kernel(const T* __restrict__ F, int Tf, int r0, int c0, int nr, int nc, T* __restrict__ out) {
    constexpr int L = Fx<T>::L;
    const long long total = (long long)nr * nc;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int r = r0 + (int)(e % nr), c = c0 + (int)(e / nr);
        out[e] = r >= c ? F[p_off(Tf << L, L, r, c)] : (T)0;
    }
}

// ---- solve / multiply: the diagonal tile ------------------------------------------------------------------------------------------
// One workgroup of 16 waves; wave w owns the right-hand sides w, w + 16, w + 32, w + 48, lane l the rows l (and l + 64 for E = 128)
// of the tile, which is read into LDS first.  SOLVE: column-oriented forward substitution, y_j = v_j / l_jj, v_i -= l_ij y_j for i > j: the chain runs over the
// columns j, the rows are the lanes.  MULTIPLY: V += tril(L_kk) Z_k, the columns j in order.
template <typename T, bool SOLVE>
__global__ __launch_bounds__(SOL_THREADS) void factor_rhs_diag_kernel(const T* __restrict__ F, int Tf, int k, int n, double* V,
                                                                       const double* __restrict__ Z, int ld, int r) {
    constexpr int L = Fx<T>::L, E = 1 << L, RP = E / 64, NQ = RHS_MAX / (SOL_THREADS / 64);
    __shared__ T tile[E * E];                                             // L_kk: the chain over j reads LDS, not memory
    {
        const T* __restrict__ g = F + tile_base(k, k, Tf, L);
        for (int e = threadIdx.x; e < E * E; e += SOL_THREADS) tile[e] = g[e];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = n - (k << L) < E ? n - (k << L) : E;
    double v[NQ][RP];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int p = 0; p < RP; ++p) {
            const int c = wave + (SOL_THREADS / 64) * q, row = lane + 64 * p;
            v[q][p] = (c < r && row < m) ? V[(size_t)c * ld + (k << L) + row] : 0.0;
        }
    for (int j = 0; j < m; ++j) {
        double lj[RP];
#pragma unroll
        for (int p = 0; p < RP; ++p) lj[p] = (double)tile[j * E + lane + 64 * p];
        if (SOLVE) {
            double ljj = __shfl(lj[0], j & 63);
            if (RP > 1) {
                const double hi = __shfl(lj[RP - 1], j & 63);
                ljj = (j >> 6) ? hi : ljj;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                double vj = __shfl(v[q][0], j & 63);
                if (RP > 1) {
                    const double hi = __shfl(v[q][RP - 1], j & 63);
                    vj = (j >> 6) ? hi : vj;
                }
                const double y = vj / ljj;
#pragma unroll
                for (int p = 0; p < RP; ++p) {
                    const int row = lane + 64 * p;
                    if (row > j) v[q][p] -= lj[p] * y;
                    else if (row == j) v[q][p] = y;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = wave + (SOL_THREADS / 64) * q;
                const double zj = c < r ? Z[(size_t)c * ld + (k << L) + j] : 0.0;
#pragma unroll
                for (int p = 0; p < RP; ++p)
                    if (lane + 64 * p >= j) v[q][p] += lj[p] * zj;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int p = 0; p < RP; ++p) {
            const int c = wave + (SOL_THREADS / 64) * q, row = lane + 64 * p;
            if (c < r && row < m) V[(size_t)c * ld + (k << L) + row] = v[q][p];
        }
}

// ---- solve / multiply: the tile column below the diagonal tile ------------------------------------------------------------------
// dst_I += sign L_Ik src_k for the tiles I > k, a workgroup per tile (striding), src_k (E x 64 doubles) in LDS.  Thread: row
// t mod E of the tile and NC of the right-hand sides; the sum runs over the tile's columns j in order.
template <typename T>
__global__ __launch_bounds__(256) void factor_rhs_col_kernel(const T* __restrict__ F, int Tf, int k, int Tn, int n, double* dst,
                                                              const double* src, int ld, int r, double sign) {
    constexpr int L = Fx<T>::L, E = 1 << L, NC = RHS_MAX / (256 >> L);
    __shared__ double sY[E * RHS_MAX];
    for (int e = threadIdx.x; e < E * RHS_MAX; e += 256) {
        const int j = e & (E - 1), c = e >> L;
        sY[j * RHS_MAX + c] = c < r ? src[(size_t)c * ld + (k << L) + j] : 0.0;
    }
    __syncthreads();
    const int rl = threadIdx.x & (E - 1), cbase = (threadIdx.x >> L) * NC;
    for (int I = k + 1 + (int)blockIdx.x; I < Tn; I += gridDim.x) {
        const T* __restrict__ tile = F + tile_base(I, k, Tf, L);
        double acc[NC];
#pragma unroll
        for (int ci = 0; ci < NC; ++ci) acc[ci] = 0.0;
        for (int j0 = 0; j0 < E; j0 += 16) {                               // sixteen loads in flight, then their products
            T lv[16];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) lv[jj] = tile[(j0 + jj) * E + rl];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const double l = (double)lv[jj];
#pragma unroll
                for (int ci = 0; ci < NC; ++ci) acc[ci] += l * sY[(j0 + jj) * RHS_MAX + cbase + ci];
            }
        }
        const int row = (I << L) + rl;
        if (row < n) {
#pragma unroll
            for (int ci = 0; ci < NC; ++ci)
                if (cbase + ci < r) dst[(size_t)(cbase + ci) * ld + row] += sign * acc[ci];
        }
    }
}

inline unsigned grid_of(long long items) { return (unsigned)(items < 1 ? 1 : (items < GRID_MAX ? items : GRID_MAX)); }

// the whole factorisation, enqueued on f's stream; the copy-in has been enqueued
template <typename T>
int enqueue_factor(slam_ekf_factor* f, int n) {
    constexpr int L = Fx<T>::L, E = 1 << L;
    T* F = (T*)f->F;
    const int Tn = (n + E - 1) >> L, Tf = f->Tf, pt = f->pt;
    for (int k0 = 0; k0 < Tn; k0 += pt) {
        const int k1 = k0 + pt < Tn ? k0 + pt : Tn;
        for (int k = k0; k < k1; ++k) {
            hipLaunchKernelGGL(factor_diag_kernel<T>, dim3(1), dim3(DIAG_THREADS), 0, f->stream, F, Tf, k, n, f->stat);
            if (k + 1 < Tn)
                hipLaunchKernelGGL(factor_panel_kernel<T>, dim3(grid_of(Tn - k - 1)), dim3(E), 0, f->stream, F, Tf, k, Tn, f->stat);
            if (k + 1 < k1) {                                             // the rest of the panel, from the one finished column
                long long items = 0;
                for (int J = k + 1; J < k1; ++J) items += Tn - J;
                hipLaunchKernelGGL(factor_trail_kernel<T>, dim3(grid_of(items)), dim3(256), 0, f->stream, F, Tf, Tn, k, k + 1, k + 1, k1,
                                   items, f->stat);
            }
        }
        if (k1 < Tn) {                                                    // everything to the right, from the whole panel
            const long long items = (long long)(Tn - k1) * (Tn - k1 + 1) / 2;
            hipLaunchKernelGGL(factor_trail_kernel<T>, dim3(grid_of(items)), dim3(256), 0, f->stream, F, Tf, Tn, k0, k1, k1, Tn, items,
                               f->stat);
        }
        HIP_TRY(hipGetLastError());
    }
    return SLAM_OK;
}

template <typename T, typename S>
int enqueue_copyin(slam_ekf_factor* f, const slam_ekf* src, int n) {
    constexpr int L = Fx<T>::L, E = 1 << L;
    const int Tn = (n + E - 1) >> L;
    const long long items = (long long)Tn * (Tn + 1) / 2;
    hipLaunchKernelGGL((factor_copyin_kernel<T, S>), dim3(grid_of(items)), dim3(256), 0, f->stream, (T*)f->F, f->Tf, (const S*)src->P, src->ld, n,
                       Tn, items);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(factor_x_kernel<S>, dim3((n + 255) / 256), dim3(256), 0, f->stream, f->xd, (const S*)src->x, n);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

void fill_info(slam_ekf_factor* f, int n, int status) {
    const int Tn = (n + f->E - 1) >> f->L;
    double* o = f->info;
    for (int i = 0; i < 8; ++i) o[i] = 0.0;
    o[0] = n;
    o[1] = status;
    o[2] = -1.0;
    o[7] = f->pt;
    if (status == SLAM_E_NOTPD) {
        o[2] = f->hstat[1];
        o[3] = f->hstat[2];
    } else if (status == SLAM_OK) {
        double mn = INFINITY, mx = 0.0, ls = 0.0;
        for (int k = 0; k < Tn; ++k) {
            const double* s = f->hstat.data() + 8 + 3 * k;
            mn = s[0] < mn ? s[0] : mn;
            mx = s[1] > mx ? s[1] : mx;
            ls += s[2];
        }
        o[4] = mn;
        o[5] = mx;
        o[6] = 2.0 * ls;
    }
}

int check_ready(slam_ekf_factor* f) {
    ARG_CHECK(f != nullptr, "null handle");
    ARG_CHECK(f->valid, "the factor holds no factorisation (never computed, or the last compute failed)");
    return SLAM_OK;
}

int ensure_rhs(slam_ekf_factor* f) {
    const size_t bytes = sizeof(double) * (size_t)f->Tf * f->E * RHS_MAX;
    if (!f->dB) HIP_TRY(hipMalloc((void**)&f->dB, bytes));
    if (!f->dZ) HIP_TRY(hipMalloc((void**)&f->dZ, bytes));
    return SLAM_OK;
}

// the walk over tile columns: V (and Z for multiply) are on the device with leading dimension ld
template <typename T, bool SOLVE>
int enqueue_walk(slam_ekf_factor* f, int r) {
    constexpr int L = Fx<T>::L, E = 1 << L;
    const int n = f->n, Tn = (n + E - 1) >> L, ld = f->Tf * E;
    const T* F = (const T*)f->F;
    for (int k = 0; k < Tn; ++k) {
        hipLaunchKernelGGL((factor_rhs_diag_kernel<T, SOLVE>), dim3(1), dim3(SOL_THREADS), 0, f->stream, F, f->Tf, k, n, f->dB, f->dZ, ld, r);
        if (k + 1 < Tn)
            hipLaunchKernelGGL(factor_rhs_col_kernel<T>, dim3(grid_of(Tn - k - 1)), dim3(256), 0, f->stream, F, f->Tf, k, Tn, n, f->dB,
                               SOLVE ? f->dB : f->dZ, ld, r, SOLVE ? -1.0 : 1.0);
        HIP_TRY(hipGetLastError());
    }
    return SLAM_OK;
}

int rhs_call(slam_ekf_factor* f, const double* in, int r, int ldin, double* out, bool solve) {
    int rc;
    if ((rc = check_ready(f))) return rc;
    ARG_CHECK(in != nullptr && out != nullptr, "null argument");
    ARG_CHECK(r >= 1 && r <= RHS_MAX, "r must be 1 .. 64");
    ARG_CHECK(ldin >= f->n, "leading dimension below n");
    HIP_TRY(hipSetDevice(f->device));
    if ((rc = ensure_rhs(f))) return rc;
    const int n = f->n;
    const size_t ld = (size_t)f->Tf * f->E;
    double* d_in = solve ? f->dB : f->dZ;
    HIP_TRY(hipMemcpy2DAsync(d_in, sizeof(double) * ld, in, sizeof(double) * (size_t)ldin, sizeof(double) * (size_t)n, (size_t)r,
                             hipMemcpyHostToDevice, f->stream));
    if (!solve) HIP_TRY(hipMemsetAsync(f->dB, 0, sizeof(double) * ld * (size_t)r, f->stream));
    if (f->dtype == SLAM_F32) rc = solve ? enqueue_walk<float, true>(f, r) : enqueue_walk<float, false>(f, r);
    else rc = solve ? enqueue_walk<double, true>(f, r) : enqueue_walk<double, false>(f, r);
    if (rc) return rc;
    HIP_TRY(hipMemcpy2DAsync(out, sizeof(double) * (size_t)ldin, f->dB, sizeof(double) * ld, sizeof(double) * (size_t)n, (size_t)r,
                             hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" int slam_ekf_factor_create(slam_ekf_factor_t* out, int dtype, int max_landmarks, int device, int panel_tiles) {
    ARG_CHECK(out != nullptr, "handle pointer is null");
    *out = nullptr;
    ARG_CHECK(dtype == SLAM_F32 || dtype == SLAM_F64, "dtype must be SLAM_F32 or SLAM_F64");
    ARG_CHECK(max_landmarks >= 0 && max_landmarks <= 500000, "max_landmarks out of range");
    ARG_CHECK(panel_tiles == 0 || panel_tiles == 1 || panel_tiles == 2 || panel_tiles == 4, "panel_tiles must be 0, 1, 2 or 4");
    const int ndev = slam_device_count();
    if (ndev <= 0) {
        slam_set_error("no HIP device available: libslamhip has no CPU fallback");
        return SLAM_E_HIP;
    }
    ARG_CHECK(device >= 0 && device < ndev, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    slam_ekf_factor* f = new slam_ekf_factor();
    f->dtype = dtype;
    f->device = device;
    f->maxN = max_landmarks;
    f->L = dtype == SLAM_F32 ? 7 : 6;
    f->E = 1 << f->L;
    f->Tf = (3 + 2 * max_landmarks + f->E - 1) >> f->L;
    f->esz = dtype == SLAM_F32 ? 4 : 8;
    // the default panel width per dtype: the fastest measured
    f->pt = panel_tiles ? panel_tiles : 4;
    f->F = nullptr;
    f->xd = f->stat = f->dB = f->dZ = nullptr;
    f->stream = nullptr;
    f->n = 0;
    f->valid = 0;
    for (int i = 0; i < 8; ++i) f->info[i] = 0.0;
    f->info[2] = -1.0;
    f->info[7] = f->pt;
    f->hstat.assign(8 + 3 * (size_t)f->Tf, 0.0);
    const size_t tiles = (size_t)f->Tf * ((size_t)f->Tf + 1) / 2;
    hipError_t e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&f->F, (tiles << (2 * f->L)) * f->esz);
    if (e == hipSuccess) e = hipMalloc((void**)&f->xd, sizeof(double) * (size_t)(3 + 2 * max_landmarks));
    if (e == hipSuccess) e = hipMalloc((void**)&f->stat, sizeof(double) * f->hstat.size());
    if (e != hipSuccess) {
        slam_set_error("factor: allocation failed: %s", hipGetErrorString(e));
        (void)slam_ekf_factor_destroy(f);
        return e == hipErrorOutOfMemory ? SLAM_E_NOMEM : SLAM_E_HIP;
    }
    *out = f;
    return SLAM_OK;
}

extern "C" int slam_ekf_factor_destroy(slam_ekf_factor_t f) {
    if (!f) return SLAM_OK;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    if (f->F) (void)hipFree(f->F);
    if (f->xd) (void)hipFree(f->xd);
    if (f->stat) (void)hipFree(f->stat);
    if (f->dB) (void)hipFree(f->dB);
    if (f->dZ) (void)hipFree(f->dZ);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
    return SLAM_OK;
}

extern "C" int slam_ekf_factor_compute(slam_ekf_factor_t f, slam_ekf_t src, double info[8]) {
    SLAM_RANGE();
    ARG_CHECK(f != nullptr && src != nullptr, "null handle");
    ARG_CHECK(info != nullptr, "info is null");
    ARG_CHECK(f->device == src->device, "the factor and the state live on different devices");
    ARG_CHECK(!(f->dtype == SLAM_F32 && src->dtype == SLAM_F64), "an fp32 factor of an fp64 state is not offered");
    if (src->N > f->maxN) {
        slam_set_error("factor: %d landmarks exceed capacity %d", src->N, f->maxN);
        return SLAM_E_CAPACITY;
    }
    int rc;
    if (src->pending_status && (rc = slam_ekf_sync(src))) return rc;     // src's deferred status; the factor untouched
    HIP_TRY(hipSetDevice(f->device));
    const int n = 3 + 2 * src->N;
    f->valid = 0;
    // the copy-in reads src: ordered against src's stream (after a failed launch the events still run, so that src never overtakes
    // what was enqueued)
    rc = slam_between(f->stream, src->stream, [&]() -> int {
        HIP_TRY(hipMemsetAsync(f->stat, 0, sizeof(double) * f->hstat.size(), f->stream));
        if (f->dtype == SLAM_F32) return enqueue_copyin<float, float>(f, src, n);
        if (src->dtype == SLAM_F64) return enqueue_copyin<double, double>(f, src, n);
        return enqueue_copyin<double, float>(f, src, n);
    });
    if (rc) return rc;
    if ((rc = f->dtype == SLAM_F32 ? enqueue_factor<float>(f, n) : enqueue_factor<double>(f, n))) return rc;
    f->hx.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(f->hx.data(), f->xd, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipMemcpyAsync(f->hstat.data(), f->stat, sizeof(double) * f->hstat.size(), hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(hipStreamSynchronize(f->stream));
    f->n = n;
    const int status = f->hstat[0] != 0.0 ? SLAM_E_NOTPD : SLAM_OK;
    fill_info(f, n, status);
    memcpy(info, f->info, sizeof(f->info));
    if (status == SLAM_E_NOTPD) {
        slam_set_error("factor: not positive definite: the pivot of state index %d is %g", (int)f->hstat[1], f->hstat[2]);
        return SLAM_E_NOTPD;
    }
    f->valid = 1;
    return SLAM_OK;
}

extern "C" int slam_ekf_factor_info(slam_ekf_factor_t f, double info[8]) {
    ARG_CHECK(f != nullptr && info != nullptr, "null argument");
    memcpy(info, f->info, sizeof(f->info));
    return SLAM_OK;
}

extern "C" int slam_ekf_factor_get(slam_ekf_factor_t f, int r0, int c0, int nr, int nc, void* out, int ld_out) {
    SLAM_RANGE();
    int rc;
    if ((rc = check_ready(f))) return rc;
    ARG_CHECK(r0 >= 0 && c0 >= 0 && nr >= 0 && nc >= 0, "negative block argument");
    ARG_CHECK(r0 <= f->n - nr && c0 <= f->n - nc, "block reaches beyond n");
    ARG_CHECK(ld_out >= nr, "ld_out below nr");
    if (nr == 0 || nc == 0) return SLAM_OK;
    ARG_CHECK(out != nullptr, "out is null");
    HIP_TRY(hipSetDevice(f->device));
    const size_t cnt = (size_t)nr * (size_t)nc;
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, cnt * f->esz));
    const unsigned grid = grid_of((long long)((cnt + 255) / 256));
    if (f->dtype == SLAM_F32) hipLaunchKernelGGL(factor_get_kernel<float>, dim3(grid), dim3(256), 0, f->stream, (const float*)f->F, f->Tf, r0, c0, nr, nc, (float*)d);
    else hipLaunchKernelGGL(factor_get_kernel<double>, dim3(grid), dim3(256), 0, f->stream, (const double*)f->F, f->Tf, r0, c0, nr, nc, (double*)d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(out, f->esz * (size_t)ld_out, d, f->esz * (size_t)nr, f->esz * (size_t)nr, (size_t)nc, hipMemcpyDeviceToHost, f->stream);
    const hipError_t e2 = hipStreamSynchronize(f->stream);
    (void)hipFree(d);
    HIP_TRY(e);
    HIP_TRY(e2);
    return SLAM_OK;
}

extern "C" int slam_ekf_factor_mean(slam_ekf_factor_t f, double* x) {
    int rc;
    if ((rc = check_ready(f))) return rc;
    ARG_CHECK(x != nullptr, "x is null");
    memcpy(x, f->hx.data(), sizeof(double) * (size_t)f->n);
    return SLAM_OK;
}

extern "C" int slam_ekf_factor_solve(slam_ekf_factor_t f, const double* B, int r, int ldb, double* Y, double* d2) {
    SLAM_RANGE();
    const int rc = rhs_call(f, B, r, ldb, Y, true);
    if (rc) return rc;
    if (d2)
        for (int c = 0; c < r; ++c) {
            double s = 0.0;
            for (int i = 0; i < f->n; ++i) s += Y[(size_t)c * ldb + i] * Y[(size_t)c * ldb + i];
            d2[c] = s;
        }
    return SLAM_OK;
}

extern "C" int slam_ekf_factor_multiply(slam_ekf_factor_t f, const double* Z, int r, int ldz, double* out) {
    SLAM_RANGE();
    return rhs_call(f, Z, r, ldz, out, false);
}
