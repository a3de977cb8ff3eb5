// ekf_join.hip -- map joining: the local map of handle b appended to the global map of handle a (slam_ekf_join,
// include/slamhip_join.h).
//
//     P' = F P_a F' + G P_b G',  n' = n_a + 2 N_b
// b's frame is a's vehicle pose (x, y, phi); c = cos phi, s = sin phi are the correctly rounded doubles of a's stored heading,
// formed ONCE by a one-thread launch (dd_trig.h) into words [16], [17] of a's small device scratch.  For a point p of b:
// J(p) = [1 0 j0; 0 1 j1], j0 = -(s px + c py), j1 = c px - s py, R = [c -s; s c].  Groups as in ekf_transform.hip: g = 0 the pose
// pair, g = 1 the heading, g >= 2 the landmark pair (2g - 1, 2g).  b's landmark group g lands 2 N_a state indices further in a.
//
// THE HAZARD.  The new vehicle strip P'[:, 0:3], P'[0:3, 0:3] and x'[0:3] overwrites exactly what every other value is computed
// from.  It is resolved by the ORDER OF THREE LAUNCHES on a's stream (behind the one that forms c and s), without a copy of the strip:
//   1. join_rows_kernel   writes rows >= n_a only (and x[n_a ..]): the new landmarks' rows against a's old landmark columns, against
//                         the vehicle columns 0 .. 2 (positions (r, 0 .. 2) with r >= n_a: unused before the call) and against
//                         each other.  It READS the old strip, the old 3 x 3 block and the old pose, none of which it writes.
//   2. join_vehicle_kernel  thread `col` (3 <= col < n_a) reads the three stored values P_a[col, 0:3], nobody else's, and rewrites
//                         them as J_v P_a[0:3, col] (and their mirrors inside diagonal tile 0, which nobody reads).  Reads x_a[2]
//                         and b's pose; writes neither.  The 3 x 3 block is left alone.
//   3. join_pose_kernel   one thread: reads the old 3 x 3 block, the old pose, b's 3 x 3 block and pose, writes P'[0:3, 0:3], x'[0:3].
// Within a launch no thread reads what another thread of the launch writes; across launches every reader of an old value runs in
// an earlier launch than its writer.  a's landmark-landmark part and everything from n' on is never touched.  b is only read.
//
// OWNERSHIP in join_rows_kernel (tests/join_ref.py runs this rule literally, in any thread order, and counts the writes):
//   * strip workgroups: entry pair (rows n_a + 2j, n_a + 2j + 1; column col), 3 <= col < n_a, is owned by the thread with lane = j mod 64
//     of the wave that walks col: the lanes of a wave walk the ROWS of one column (128 consecutive elements: coalesced stores), a
//     wave walks SC columns one after the other, reading P_a[col, 0:3] as three wave-uniform loads.
//   * block workgroups: the 2 x 2 (2 x 1 against the heading) destination block of b's groups (gr, gc), gr >= 2, gc <= gr, is owned
//     by one thread: thread -> gr (consecutive lanes: consecutive row pairs, so the source loads and the destination stores of a
//     column are coalesced on both sides although source and destination are offset by 2 N_a, which is no multiple of the tile
//     edge: every entry goes through p_off of its own matrix, so pairs that straddle a tile edge in b, in a, or in both need nothing
//     special); a workgroup walks CG column groups.  Row and column shift by the same amount and gr >= gc, so a stored
//     destination entry always has a stored source entry; the diagonal block gr == gc reads b01 as b10 and stores the three lower
//     entries through p_store_sym.  The thread that owns (gr, 0) also writes landmark gr's mean.
// j0 and j1 are two-term dot products that nearly cancel for a landmark abeam or ahead of the vehicle: dot2_rn (dd_trig.h) carries
// the products' rounding errors.  No LDS, no private scratch, no atomics; nothing is allocated.
#include <cmath>

#include "common.h"
#include "../../include/slamhip_join.h"
#include "device_math.h"
#include "dd_trig.h"

namespace {

constexpr int SC = 8;     // columns a strip wave walks
constexpr int CG = 4;     // column groups a block workgroup walks

// launch 0: c and s, once (dd_trig.h: the correctly rounded doubles), into two words of a's small scratch
template <typename T>
__global__ void join_trig_kernel(const T* __restrict__ xa, double* __restrict__ cs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s, c;
    sincos_rn((double)xa[2], &s, &c);
    cs[0] = c;
    cs[1] = s;
}

template <typename T>
__device__ __forceinline__ void join_strip(T* __restrict__ Pa, int lda, int nA, const double* __restrict__ cs, const T* __restrict__ xb,
                                           int NB, int bx, int by) {
    constexpr int L = kTileLog2<T>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = by * 64 + lane;
    if (j >= NB) return;
    const double c = cs[0], s = cs[1];
    const double px = (double)xb[3 + 2 * j], py = (double)xb[4 + 2 * j];
    const double j0 = -dot2_rn(s, px, c, py), j1 = dot2_rn(c, px, -s, py);
    const int r = nA + 2 * j;
    const int col0 = 3 + (bx * 4 + wave) * SC;
    for (int k = 0; k < SC; ++k) {
        const int col = col0 + k;
        if (col >= nA) break;
        const double p0 = (double)Pa[p_off(lda, L, col, 0)], p1 = (double)Pa[p_off(lda, L, col, 1)],
                     p2 = (double)Pa[p_off(lda, L, col, 2)];
        p_store_sym(Pa, lda, L, r, col, (T)(p0 + j0 * p2));
        p_store_sym(Pa, lda, L, r + 1, col, (T)(p1 + j1 * p2));
    }
}

template <typename T>
__device__ __forceinline__ void join_block(T* __restrict__ Pa, int lda, int NA, T* __restrict__ xa, const double* __restrict__ cs,
                                           const T* __restrict__ Pb, int ldb, const T* __restrict__ xb, int NB, int bx, int by) {
    constexpr int L = kTileLog2<T>;
    const int gr = 2 + bx * 256 + (int)threadIdx.x;
    if (gr >= NB + 2) return;
    const int gc0 = by * CG;
    if (gc0 > gr) return;
    const int sh = 2 * NA;
    const double c = cs[0], s = cs[1];
    const double xv = (double)xa[0], yv = (double)xa[1];
    const double v00 = (double)Pa[p_off(lda, L, 0, 0)], v10 = (double)Pa[p_off(lda, L, 1, 0)], v11 = (double)Pa[p_off(lda, L, 1, 1)],
                 v20 = (double)Pa[p_off(lda, L, 2, 0)], v21 = (double)Pa[p_off(lda, L, 2, 1)], v22 = (double)Pa[p_off(lda, L, 2, 2)];
    const int rB = grp_first(gr), rD = rB + sh;
    const double px = (double)xb[rB], py = (double)xb[rB + 1];
    const double jr0 = -dot2_rn(s, px, c, py), jr1 = dot2_rn(c, px, -s, py);
    // GP = J_gr Pvv (2 x 3), Pvv symmetric from its stored lower triangle
    const double g00 = v00 + jr0 * v20, g01 = v10 + jr0 * v21, g02 = v20 + jr0 * v22;
    const double g10 = v10 + jr1 * v20, g11 = v11 + jr1 * v21, g12 = v21 + jr1 * v22;
    for (int gc = gc0; gc < gc0 + CG && gc <= gr; ++gc) {
        if (gc == 1) {                                                    // against the heading: J = [0 0 1], R = 1
            const double b0 = (double)Pb[p_off(ldb, L, rB, 2)], b1 = (double)Pb[p_off(ldb, L, rB + 1, 2)];
            p_store_sym(Pa, lda, L, rD, 2, (T)(g02 + (c * b0 - s * b1)));
            p_store_sym(Pa, lda, L, rD + 1, 2, (T)(g12 + (s * b0 + c * b1)));
            continue;
        }
        const int qB = grp_first(gc), qD = gc < 2 ? qB : qB + sh;
        const double qx = (double)xb[qB], qy = (double)xb[qB + 1];
        const double jc0 = -dot2_rn(s, qx, c, qy), jc1 = dot2_rn(c, qx, -s, qy);
        const double b00 = (double)Pb[p_off(ldb, L, rB, qB)], b10 = (double)Pb[p_off(ldb, L, rB + 1, qB)],
                     b11 = (double)Pb[p_off(ldb, L, rB + 1, qB + 1)];
        const double b01 = gr == gc ? b10 : (double)Pb[p_off(ldb, L, rB, qB + 1)];
        const double m00 = c * b00 - s * b10, m01 = c * b01 - s * b11, m10 = s * b00 + c * b10, m11 = s * b01 + c * b11;
        const T o00 = (T)((g00 + g02 * jc0) + (c * m00 - s * m01));
        const T o10 = (T)((g10 + g12 * jc0) + (c * m10 - s * m11));
        const T o11 = (T)((g11 + g12 * jc1) + (s * m10 + c * m11));
        p_store_sym(Pa, lda, L, rD, qD, o00);
        p_store_sym(Pa, lda, L, rD + 1, qD, o10);
        p_store_sym(Pa, lda, L, rD + 1, qD + 1, o11);
        if (gr != gc) p_store_sym(Pa, lda, L, rD, qD + 1, (T)((g01 + g02 * jc1) + (s * m00 + c * m01)));
        if (gc == 0) {
            xa[rD] = (T)(xv + (c * px - s * py));
            xa[rD + 1] = (T)(yv + (s * px + c * py));
        }
    }
}

// launch 1: workgroups [0, nsx * nsy): the strip; the rest: the new block, nbx row chunks per column-group chunk
template <typename T>
__global__ __launch_bounds__(256) void join_rows_kernel(T* __restrict__ Pa, int lda, int NA, T* __restrict__ xa,
                                                         const double* __restrict__ cs, const T* __restrict__ Pb, int ldb,
                                                         const T* __restrict__ xb, int NB, int nsx, int nsy, int nbx) {
    int b = blockIdx.x;
    if (b < nsx * nsy) return join_strip<T>(Pa, lda, 3 + 2 * NA, cs, xb, NB, b % nsx, b / nsx);
    b -= nsx * nsy;
    join_block<T>(Pa, lda, NA, xa, cs, Pb, ldb, xb, NB, b % nbx, b / nbx);
}

// launch 2: a's old landmark columns against the new vehicle rows, in place, thread by thread
template <typename T>
__global__ __launch_bounds__(256) void join_vehicle_kernel(T* __restrict__ Pa, int lda, int nA, const double* __restrict__ cs,
                                                            const T* __restrict__ xb) {
    constexpr int L = kTileLog2<T>;
    const int col = 3 + blockIdx.x * 256 + (int)threadIdx.x;
    if (col >= nA) return;
    const double c = cs[0], s = cs[1];
    const double px = (double)xb[0], py = (double)xb[1];
    const double j0 = -dot2_rn(s, px, c, py), j1 = dot2_rn(c, px, -s, py);
    const T t2 = Pa[p_off(lda, L, col, 2)];
    const double p0 = (double)Pa[p_off(lda, L, col, 0)], p1 = (double)Pa[p_off(lda, L, col, 1)], p2 = (double)t2;
    p_store_sym(Pa, lda, L, col, 0, (T)(p0 + j0 * p2));
    p_store_sym(Pa, lda, L, col, 1, (T)(p1 + j1 * p2));
    p_store_sym(Pa, lda, L, col, 2, t2);                                  // the heading's row: J = [0 0 1], the stored bits again
}

// launch 3: the vehicle's own 3 x 3 block and the pose
template <typename T>
__global__ void join_pose_kernel(T* __restrict__ Pa, int lda, T* __restrict__ xa, const double* __restrict__ cs,
                                 const T* __restrict__ Pb, int ldb, const T* __restrict__ xb) {
    constexpr int L = kTileLog2<T>;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double phi = (double)xa[2];
    const double c = cs[0], s = cs[1];
    const double xv = (double)xa[0], yv = (double)xa[1];
    const double px = (double)xb[0], py = (double)xb[1], phib = (double)xb[2];
    const double j0 = -dot2_rn(s, px, c, py), j1 = dot2_rn(c, px, -s, py);
    const double v00 = (double)Pa[p_off(lda, L, 0, 0)], v10 = (double)Pa[p_off(lda, L, 1, 0)], v11 = (double)Pa[p_off(lda, L, 1, 1)],
                 v20 = (double)Pa[p_off(lda, L, 2, 0)], v21 = (double)Pa[p_off(lda, L, 2, 1)], v22 = (double)Pa[p_off(lda, L, 2, 2)];
    const double b00 = (double)Pb[p_off(ldb, L, 0, 0)], b10 = (double)Pb[p_off(ldb, L, 1, 0)], b11 = (double)Pb[p_off(ldb, L, 1, 1)],
                 b20 = (double)Pb[p_off(ldb, L, 2, 0)], b21 = (double)Pb[p_off(ldb, L, 2, 1)], b22 = (double)Pb[p_off(ldb, L, 2, 2)];
    const double g00 = v00 + j0 * v20, g02 = v20 + j0 * v22;
    const double g10 = v10 + j1 * v20, g11 = v11 + j1 * v21, g12 = v21 + j1 * v22;
    const double m00 = c * b00 - s * b10, m01 = c * b10 - s * b11, m10 = s * b00 + c * b10, m11 = s * b10 + c * b11;
    p_store_sym(Pa, lda, L, 0, 0, (T)((g00 + g02 * j0) + (c * m00 - s * m01)));
    p_store_sym(Pa, lda, L, 1, 0, (T)((g10 + g12 * j0) + (c * m10 - s * m11)));
    p_store_sym(Pa, lda, L, 1, 1, (T)((g11 + g12 * j1) + (s * m10 + c * m11)));
    p_store_sym(Pa, lda, L, 2, 0, (T)((v20 + v22 * j0) + (c * b20 - s * b21)));
    p_store_sym(Pa, lda, L, 2, 1, (T)((v21 + v22 * j1) + (s * b20 + c * b21)));
    p_store_sym(Pa, lda, L, 2, 2, (T)(v22 + b22));
    xa[0] = (T)(xv + (c * px - s * py));
    xa[1] = (T)(yv + (s * px + c * py));
    xa[2] = (T)mpi_to_pi_d(phi + phib);
}

template <typename T>
int join_impl(slam_ekf* a, const slam_ekf* b) {
    const int NA = a->N, NB = b->N, nA = 3 + 2 * NA;
    T* Pa = (T*)a->P;
    T* xa = (T*)a->x;
    const T* Pb = (const T*)b->P;
    const T* xb = (const T*)b->x;
    double* cs = a->d_small + 16;                                        // [16], [17]: used by no other call (common.h)
    hipLaunchKernelGGL(join_trig_kernel<T>, dim3(1), dim3(64), 0, a->stream, (const T*)xa, cs);
    HIP_TRY(hipGetLastError());
    if (NB > 0) {
        const int nsx = NA > 0 ? (nA - 3 + 4 * SC - 1) / (4 * SC) : 0, nsy = (NB + 63) / 64;
        const int nbx = (NB + 255) / 256, nby = (NB + 2 + CG - 1) / CG;
        const long long blocks = (long long)nsx * nsy + (long long)nbx * nby;
        hipLaunchKernelGGL(join_rows_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, a->stream, Pa, a->ld, NA, xa, cs, Pb, b->ld, xb, NB, nsx,
                           nsy, nbx);
        HIP_TRY(hipGetLastError());
    }
    if (NA > 0) {
        hipLaunchKernelGGL(join_vehicle_kernel<T>, dim3((nA - 3 + 255) / 256), dim3(256), 0, a->stream, Pa, a->ld, nA, cs, xb);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(join_pose_kernel<T>, dim3(1), dim3(64), 0, a->stream, Pa, a->ld, xa, cs, Pb, b->ld, xb);
    HIP_TRY(hipGetLastError());
    return SLAM_OK;
}

}  // namespace

/* Map joining (slamhip_join.h): b appended to a in a's frame, enqueued on a's stream between two events that order it against b's. */
extern "C" int slam_ekf_join(slam_ekf_t a, slam_ekf_t b, int32_t* first_new) {
    SLAM_RANGE();
    ARG_CHECK(a != nullptr && b != nullptr, "null handle");
    ARG_CHECK(a != b, "a map cannot be joined into itself");
    ARG_CHECK(a->dtype == b->dtype, "the two maps differ in dtype");
    ARG_CHECK(a->device == b->device, "the two maps live on different devices");
    if (a->N + b->N > a->maxN) {
        slam_set_error("join: %d + %d landmarks exceed capacity %d", a->N, b->N, a->maxN);
        return SLAM_E_CAPACITY;
    }
    int rc;
    if (b->pending_status && (rc = slam_ekf_sync(b))) return rc;         // b's deferred status; a untouched
    HIP_TRY(hipSetDevice(a->device));
    // (after a failed launch slam_between's events still run, so that b never overtakes what was enqueued; a launch that fails half
    //  way leaves a's state undefined, as slamhip_join.h says)
    return slam_between(a->stream, b->stream, [&]() -> int {
        const int NA = a->N;
        const int rcj = a->dtype == SLAM_F32 ? join_impl<float>(a, b) : join_impl<double>(a, b);
        if (rcj) return rcj;
        // the launches have gone out: the host side follows the device at once, whatever the event calls behind them return
        if (first_new) *first_new = NA + 1;
        a->N = NA + b->N;
        a->grid_force = 1;                                               // the grid belongs to the old means and the old count
        a->pmax_valid = 0;                                               // new variances, and the vehicle's enter every one
        return launch_side_rebuild(a);                                   // the packed 2 x 2 diagonal blocks follow the matrix
    });
}
