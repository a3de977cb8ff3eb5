// ekf_transform.hip -- map management: the state expressed in another frame, IN PLACE (slam_ekf_transform).
//
//     p <- R p + t for the vehicle and every landmark,  phi <- mpi_to_pi(phi + theta),  P <- T P T',  T = blockdiag(R, 1, R, R, ...)
// R = [c -s; s c], c and s evaluated once on the host.  The state indices fall into GROUPS: g = 0 the pose pair (0, 1), g = 1
// the heading (2) alone, g >= 2 the landmark pair (2g - 1, 2g).  The block of P with the rows of group gr and the columns of
// group gc becomes R_r B R_c' (R_g = 1 for the heading) and depends on nothing but itself: one in-place pass, no ordering
// between blocks.  Every block with gr >= gc is OWNED by exactly one thread, which reads all of its entries (from stored
// positions r >= c only) before it writes any; a mirrored position inside a diagonal tile is written by the owner of the
// entry below the diagonal from the same value (p_store_sym), and no thread USES a value another thread writes (one load is
// wider than what is used: lane 0 of a tile's wave loads rows (0, 1) as one vector and takes row 1 only; row 0, which the
// owner of the block above may be writing, is discarded).
//
// A landmark pair starts at an ODD index, so the pair with f + 1 a multiple of the tile edge E straddles two tiles, and a
// block can lie in one, two or four stored tiles.  With h(g) = the tile row of a group's FIRST index the owner is:
//   * h(gr) == h(gc):                           transform_diag, a few workgroups per diagonal tile D, entry by entry.  This
//       takes the blocks inside tile (D, D), those that hang out of its bottom edge into tile (D + 1, D), and the straddling
//       pair's own diagonal block, whose upper entry exists only as its mirror (read b01 = b10, write the three lower ones).
//   * h(gr) > h(gc), gc straddles or gc < 2:    transform_cols, one thread per block down the column pair (coalesced
//       along the rows); entry by entry, so a row group that straddles as well needs nothing special.
//   * everything else (h(gr) > h(gc), gc a whole pair inside band J = h(gc)):  transform_tile, the vectorised pass.
//       One workgroup per tile (I, J), I > J.  A wave takes the column pair (cl, cl + 1), cl odd: lane q loads rows
//       (2q, 2q + 1) of both 512-byte columns as one 8-byte (fp32) / 16-byte (fp64, two column pairs per wave) vector, takes
//       row 2q + 2 from lane q + 1 (the one-element misalignment of the pairs is bridged by this lane exchange), computes the
//       block of rows (2q + 1, 2q + 2), hands the new row 2q + 2 to lane q + 1 and stores rows (2q, 2q + 1) as a vector again.
//       The last lane's partner row is row 0 of tile (I + 1, J), the next tile in memory: it owns the block that straddles
//       the bottom edge and stores that one element by itself; lane 0 consequently stores row 1 only -- row 0 belongs to the
//       workgroup of tile (I - 1, J), or to the diagonal kernel when I - 1 == J.
// n = 3 + 2N is odd, so a pair is either wholly below n or wholly padding: padding is never read into a result and never
// written.  The three sets touch disjoint entries and use nothing another thread writes, so ONE launch (transform_P_kernel)
// runs them side by side.  tests/test_transform_ref_cpu.py runs this rule literally (E = 4, 8), in any thread order, and counts
// the writes.
#include <cmath>

#include "common.h"
#include "../../include/slamhip_frame.h"
#include "device_math.h"

namespace {

// the block (gr, gc), gr >= gc, entry by entry through p_off / p_store_sym
template <typename T>
__device__ __forceinline__ void transform_block(T* __restrict__ P, int ld, int L, int gr, int gc, double c, double s) {
    const int r = grp_first(gr), q = grp_first(gc), nr = grp_size(gr), nc = grp_size(gc);
    if (gr == gc) {
        if (nr == 1) return;                                              // P[2, 2]: unchanged bit for bit
        const double b00 = (double)P[p_off(ld, L, r, r)], b10 = (double)P[p_off(ld, L, r + 1, r)],
                     b11 = (double)P[p_off(ld, L, r + 1, r + 1)];
        const double m00 = c * b00 - s * b10, m01 = c * b10 - s * b11, m10 = s * b00 + c * b10, m11 = s * b10 + c * b11;
        p_store_sym(P, ld, L, r, r, (T)(c * m00 - s * m01));
        p_store_sym(P, ld, L, r + 1, r, (T)(c * m10 - s * m11));
        p_store_sym(P, ld, L, r + 1, r + 1, (T)(s * m10 + c * m11));
        return;
    }
    double b[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int i = 0; i < nr; ++i)
        for (int j = 0; j < nc; ++j) b[i][j] = (double)P[p_off(ld, L, r + i, q + j)];
    double m[2][2];
    for (int j = 0; j < 2; ++j) {
        m[0][j] = nr == 2 ? c * b[0][j] - s * b[1][j] : b[0][j];
        m[1][j] = s * b[0][j] + c * b[1][j];
    }
    for (int i = 0; i < nr; ++i) {
        p_store_sym(P, ld, L, r + i, q, (T)(nc == 2 ? c * m[i][0] - s * m[i][1] : m[i][0]));
        if (nc == 2) p_store_sym(P, ld, L, r + i, q + 1, (T)(s * m[i][0] + c * m[i][1]));
    }
}

// groups whose first index lies in tile row D: [lo, hi]
__host__ __device__ inline void grp_range(int D, int L, int NG, int* lo, int* hi) {
    const int half = 1 << (L - 1);
    *lo = D == 0 ? 0 : D * half + 1;
    const int h = (D + 1) * half;
    *hi = h < NG - 1 ? h : NG - 1;
}

constexpr int DIAG_SPLIT = 8;          // workgroups per diagonal tile (its ~2000 blocks are scattered 4-entry accesses: latency)

// h(gr) == h(gc) == D; workgroup b: part b % DIAG_SPLIT of diagonal tile b / DIAG_SPLIT
template <typename T>
__device__ __forceinline__ void transform_diag(T* __restrict__ P, int ld, int NG, double c, double s, int b) {
    constexpr int L = kTileLog2<T>;
    int lo, hi;
    grp_range(b / DIAG_SPLIT, L, NG, &lo, &hi);
    const int K = hi - lo + 1;
    for (int i = (b % DIAG_SPLIT) * 256 + threadIdx.x; i < K * K; i += 256 * DIAG_SPLIT) {
        const int kc = i / K, kr = i - kc * K;                            // (consecutive threads: consecutive row groups)
        if (kr >= kc) transform_block(P, ld, L, lo + kr, lo + kc, c, s);
    }
}

// y < 2: gc = the pose pair / the heading; otherwise gc = the pair that straddles bands J, J + 1 (J = y - 2);
// row groups: every one with h(gr) > h(gc), 256 per workgroup (bx)
template <typename T>
__device__ __forceinline__ void transform_cols(T* __restrict__ P, int ld, int NG, double c, double s, int bx, int y) {
    constexpr int L = kTileLog2<T>;
    constexpr int half = 1 << (L - 1);
    const int gc = y < 2 ? y : (y - 1) * half;
    const int D = y < 2 ? 0 : y - 2;
    const int gr = (D + 1) * half + 1 + bx * 256 + threadIdx.x;           // the first group of tile row D + 1 onwards
    if (gc >= NG || gr >= NG) return;
    transform_block(P, ld, L, gr, gc, c, s);
}

// the stored tiles below the diagonal, band after band as they lie in memory: number t -> (I, J), I > J; band J holds Tu - 1 - J
__host__ __device__ inline int tri_off(int J, int Tu) { return J * (Tu - 1) - J * (J - 1) / 2; }
__host__ __device__ inline void tri_tile(int t, int Tu, int* I, int* J) {
    const double w = 2.0 * Tu - 1.0;
    int j = (int)((w - sqrt(w * w - 8.0 * t)) * 0.5);                     // an estimate; the two loops make it exact
    j = j < 0 ? 0 : (j > Tu - 2 ? Tu - 2 : j);
    while (j > 0 && tri_off(j, Tu) > t) --j;
    while (tri_off(j + 1, Tu) <= t) ++j;                                  // (tri_off(Tu - 1) is the tile count: t is below it)
    *J = j;
    *I = j + 1 + (t - tri_off(j, Tu));
}

template <typename T> struct Pair;
template <> struct Pair<float> { typedef float2 type; };
template <> struct Pair<double> { typedef double2 type; };

// tile (I, J), I > J
template <typename T>
__device__ __forceinline__ void transform_tile(T* __restrict__ P, int ld, int n, double c, double s, int I, int J) {
    typedef typename Pair<T>::type V;
    constexpr int L = kTileLog2<T>;
    constexpr int E = 1 << L, LPC = E / 2, CPW = 64 / LPC;               // lanes per column pair, column pairs per wave
    if ((I << L) >= n) return;
    T* __restrict__ tile = P + tile_base(I, J, ld >> L, L);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane & (LPC - 1), sub = lane / LPC;
    const int r0 = (I << L) + 2 * q;                                      // this lane's vector: rows r0, r0 + 1
    const bool own = r0 + 2 < n;                                          // its block: rows r0 + 1, r0 + 2
    const bool up = q > 0 && r0 < n;                                      // row r0 comes from lane q - 1's block
    const bool last = q == LPC - 1;
    const int cl0 = J == 0 ? 3 : 1;                                       // (band 0: columns 0 .. 2 are the pose groups')
    const int npairs = (E - 1 - cl0) / 2;
    for (int k0 = wave * CPW; k0 < npairs; k0 += 4 * CPW) {
        const int k = k0 + sub;
        const bool act = k < npairs;
        T* __restrict__ col = tile + ((size_t)(cl0 + 2 * (act ? k : 0)) << L);
        V a, b;
        a.x = a.y = b.x = b.y = (T)0;
        if (act) {                                                        // (the idle half of an fp64 wave loads nothing)
            a = *reinterpret_cast<const V*>(col + 2 * q);
            b = *reinterpret_cast<const V*>(col + E + 2 * q);
        }
        T ta = (T)0, tb = (T)0;
        if (act && last && own) { ta = col[(size_t)E * E]; tb = col[(size_t)E * E + E]; }     // row 0 of tile (I + 1, J)
        const T na = __shfl_down(a.x, 1), nb = __shfl_down(b.x, 1);
        const double b00 = (double)a.y, b01 = (double)b.y, b10 = (double)(last ? ta : na), b11 = (double)(last ? tb : nb);
        const double m00 = c * b00 - s * b10, m01 = c * b01 - s * b11, m10 = s * b00 + c * b10, m11 = s * b01 + c * b11;
        const T o00 = (T)(c * m00 - s * m01), o01 = (T)(s * m00 + c * m01);
        const T o10 = (T)(c * m10 - s * m11), o11 = (T)(s * m10 + c * m11);
        const T ua = __shfl_up(o10, 1), ub = __shfl_up(o11, 1);
        if (!act) continue;
        if (own && up) {
            V va, vb;
            va.x = ua; va.y = o00; vb.x = ub; vb.y = o01;
            *reinterpret_cast<V*>(col + 2 * q) = va;
            *reinterpret_cast<V*>(col + E + 2 * q) = vb;
        } else if (own) {
            col[2 * q + 1] = o00; col[E + 2 * q + 1] = o01;
        } else if (up) {
            col[2 * q] = ua; col[E + 2 * q] = ub;
        }
        if (last && own) { col[(size_t)E * E] = o10; col[(size_t)E * E + E] = o11; }
    }
}

// ONE launch for the whole of P: the three owner sets touch disjoint entries, so their workgroups need no order among them.
// Workgroups [0, nd): the diagonal tiles' parts (first: few and latency-bound, they run beside the stream of tiles);
// [nd, nd + nc): the column pairs, cx workgroups each; the rest: the tiles (I, J), I > J, band after band as they lie in memory.
template <typename T>
__global__ __launch_bounds__(256) void transform_P_kernel(T* __restrict__ P, int ld, int n, int NG, int Tu, int cx, double c, double s) {
    int b = blockIdx.x;
    const int nd = Tu * DIAG_SPLIT, nc = Tu > 1 ? (Tu + 1) * cx : 0;
    if (b < nd) return transform_diag<T>(P, ld, NG, c, s, b);
    b -= nd;
    if (b < nc) return transform_cols<T>(P, ld, NG, c, s, b % cx, b / cx);
    b -= nc;
    int I, J;
    tri_tile(b, Tu, &I, &J);
    transform_tile<T>(P, ld, n, c, s, I, J);
}

// x: one thread per group
template <typename T>
__global__ __launch_bounds__(256) void transform_x_kernel(T* __restrict__ x, int NG, double c, double s, double tx, double ty,
                                                           double theta) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= NG) return;
    if (g == 1) {
        x[2] = (T)mpi_to_pi_d((double)x[2] + theta);
        return;
    }
    const int f = grp_first(g);
    const double px = (double)x[f], py = (double)x[f + 1];
    x[f] = (T)(c * px - s * py + tx);
    x[f + 1] = (T)(s * px + c * py + ty);
}

template <typename T>
int transform_impl(slam_ekf* h, double c, double s, double tx, double ty, double theta, bool rotate) {
    constexpr int L = kTileLog2<T>;
    const int NG = h->N + 2, n = 3 + 2 * h->N;
    hipLaunchKernelGGL(transform_x_kernel<T>, dim3((NG + 255) / 256), dim3(256), 0, h->stream, (T*)h->x, NG, c, s, tx, ty, theta);
    HIP_TRY(hipGetLastError());
    if (!rotate) return SLAM_OK;                                          // R = I: P is its own image
    const int Tu = ((n - 1) >> L) + 1;                                    // tile rows that hold state
    const int cx = (NG + 255) / 256;
    const long long blocks = (long long)Tu * DIAG_SPLIT + (Tu > 1 ? (long long)(Tu + 1) * cx + (long long)Tu * (Tu - 1) / 2 : 0);
    hipLaunchKernelGGL(transform_P_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, h->stream, (T*)h->P, h->ld, n, NG, Tu, cx, c, s);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

}  // namespace

/* Map management (slamhip_frame.h): the rigid frame change (tx, ty, theta) of the whole state, in place, enqueued. */
extern "C" int slam_ekf_transform(slam_ekf_t h, double tx, double ty, double theta) {
    SLAM_RANGE();
    ARG_CHECK(h != nullptr, "null handle");
    ARG_CHECK(std::isfinite(tx) && std::isfinite(ty) && std::isfinite(theta), "tx, ty and theta must be finite");
    theta = remainder(theta, 2.0 * SLAM_PI_D);
    const double c = cos(theta), s = sin(theta);
    HIP_TRY(hipSetDevice(h->device));
    const bool rotate = !(c == 1.0 && s == 0.0);
    int rc;
    if (h->dtype == SLAM_F32) rc = transform_impl<float>(h, c, s, tx, ty, theta, rotate);
    else rc = transform_impl<double>(h, c, s, tx, ty, theta, rotate);
    if (rc) return rc;
    h->grid_force = 1;                                      // the grid belongs to the old means (the forced rebuild folds and
                                                            // clears the updates' pending displacement slots, as after an upload)
    if (!rotate) return SLAM_OK;                            // a translation moves no variance: side array and bound still hold
    h->pmax_valid = 0;                                      // the largest landmark variance changes under rotation
    return launch_side_rebuild(h);                          // the packed 2 x 2 diagonal blocks follow the matrix
}
