/* slamhip_factor.h -- the Cholesky factor of an EKF state's covariance on the device: a definiteness check, log det P, the
 * whitening solve behind the NEES, and the product behind joint samples.  The entry points of the EXTENSION library
 * libslamhip_factor.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_factor.so is built from csrc/ekf_factor.hip by the same Makefile, links against libslamhip.so (it reads
 * that library's handles and calls its internal helpers: both come from one tree and one make) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message.  The header lives in
 * include/ext/ and is found through the same -I as the others.
 *
 * THE FACTOR OBJECT owns a buffer in the state's own layout (slam_ekf_device_ptrs): tile-major, block lower, tile edge E = 128
 * (SLAM_F32) / 64 (SLAM_F64), tile (I, J), I >= J, at block number J T - J (J - 1) / 2 + (I - J) with T = the tile rows of the
 * factor's OWN capacity, ceil((3 + 2 max_landmarks) / E); all offsets are 64-bit.  It also owns a stream, a double copy of x and
 * a small device status block.  dtype is the arithmetic AND storage type of L.  It may be the source's dtype, or SLAM_F64 over a
 * SLAM_F32 source: the copy-in converts every entry exactly and re-tiles 128 -> 64 entry by entry, which makes the fp64 factor the
 * trustworthy check of an fp32 state.
 *
 * THE RULE (tests/factor_ref.py runs it literally).  n = 3 + 2 N of src, A = P[0 : n, 0 : n] read from the STORED LOWER entries:
 * A[r, c] = A[c, r] = the value stored for (max(r, c), min(r, c)) -- below the diagonal tiles the one stored value, inside a
 * diagonal tile the lower one (the convention of slam_ekf_state_written).  For i = 0 .. n - 1 in this order
 *     d_i  = a_ii - sum_{j < i} l_ij^2                          the pivot, in the factor's dtype
 *     d_i <= 0 or not finite (NaN, Inf):  column i FAILS; i is the first failing index, d_i the failing pivot, the factorisation
 *                                         stops and the call returns SLAM_E_NOTPD
 *     l_ii = sqrt(d_i),   l_ri = (a_ri - sum_{j < i} l_rj l_ij) / l_ii   for r > i        (a division, no reciprocal)
 * every operation rounded once to the factor's dtype; the ORDER in which a sum's terms are added is the device's own (tile by
 * tile on the matrix cores, then inside the diagonal tile), fixed for a given panel_tiles, so results are bit-identical from run
 * to run.  Whatever the order, |L L' - A|_ij <= gamma_(n+1) (|L| |L|')_ij with gamma_k = k u / (1 - k u), u = 2^-24 / 2^-53
 * (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3).  Rows and columns >= n of the last tile are padding: they
 * are never pivots and stay +0.0.  A second compute on the same object rewrites every tile it uses, so nothing a larger state
 * left behind is seen.
 *
 * THE ALGORITHM is a blocked right-looking Cholesky over the tile grid; the panel is panel_tiles tile columns wide.  Three kernel
 * families, every dependency a launch boundary, no workgroup ever waits for another:
 *     diag   one workgroup factors the E x E diagonal tile in LDS, stops at the first failing pivot and at n, and writes the
 *            tile's smallest and largest l_ii and its sum of log l_ii (double, in column order)
 *     panel  L_Ik = A_Ik L_kk^-T for all I > k by substitution, one workgroup per tile, L_kk in LDS
 *     trail  A_IJ -= sum_{p0 <= p < p1} L_Ip L_Jp' for the targets J0 <= J < J1, I >= J: the sum over p in registers on the matrix
 *            cores in the factor's own precision (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, no bf16 split), each target
 *            read and written once per launch.  Inside a panel: a one-tile source, the targets are the rest of the panel.  After
 *            a panel: the whole panel is the source, everything to its right the target.  Of a diagonal target only the lower
 *            triangle is meaningful.
 * When a pivot fails a flag in the device status block makes every later launch of the sequence return at once.
 *
 * info[8] of compute / info:
 *     [0] n                                 [1] the status (SLAM_OK, SLAM_E_NOTPD)
 *     [2] the first failing state index, or -1       [3] the failing pivot d_i (0 when none failed)
 *     [4] the smallest l_ii                 [5] the largest l_ii
 *     [6] log det P = 2 sum_i log l_ii: log in double per column, summed in double in column order inside a tile, the tiles'
 *         sums then added in tile order
 *     [7] panel_tiles used
 * After SLAM_E_NOTPD [4] .. [6] are 0 and the object is INVALID: get / mean / solve / multiply return SLAM_E_BADARG until a
 * compute succeeds.  The same holds for an object that has never been computed.
 *
 * Decided before anything is enqueued, src and the factor unchanged bit for bit:
 *   SLAM_E_BADARG    a null handle or null info; different devices; an fp32 factor over an fp64 source
 *   SLAM_E_CAPACITY  N of src exceeds the factor's max_landmarks
 * SLAM_E_HIP from the runtime once work has been enqueued: the factor is invalid.
 * Ordering of compute, exactly as slam_ekf_copy: src's deferred asynchronous status is resolved first, as slam_ekf_sync(src)
 * would (an error of src is returned, the factor is untouched).  The work is enqueued on the factor's stream behind an event
 * recorded on src's stream; an event recorded on the factor's stream after the last read of src (the copy-in) is made a
 * dependency of src's stream, so src may be written or destroyed as soon as the call returns.  src is only read.  compute reads
 * info back and therefore SYNCHRONISES the factor's stream (not src's).
 *
 * THE READ-OUTS work on the factor alone and synchronise, since they return host arrays.
 *   solve     Y = L^-1 B by forward substitution, B and Y n x r doubles, column-major with leading dimension ldb >= n (Y may be
 *             B), 1 <= r <= 64, and d2[c] = sum_i Y[i, c]^2 added in double in row order on the host: the NEES of error vector c.
 *             L is read in its dtype; every product and sum is fp64.
 *   multiply  out = L Z under the same conventions (ldz for both): with z ~ N(0, I) the columns x + L z are joint samples.  The
 *             library generates no random numbers.
 *   Both walk the tile columns k = 0, 1, ...: a one-workgroup kernel on the diagonal tile (solve: Y_k = L_kk^-1 B_k; multiply:
 *   out_k += tril(L_kk) Z_k), then one launch over the tile column below it (solve: B_I -= L_Ik Y_k; multiply: out_I += L_Ik Z_k,
 *   I > k), each workgroup owning the rows of one tile: nothing but launch boundaries between steps, and every sum in a fixed
 *   order.
 */
#ifndef SLAMHIP_FACTOR_H
#define SLAMHIP_FACTOR_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slam_ekf_factor* slam_ekf_factor_t;

/* panel_tiles: 1, 2 or 4 tile columns per panel, 0 = the default for the dtype; anything else SLAM_E_BADARG.
 * dtype, max_landmarks and device as slam_ekf_create. */
int slam_ekf_factor_create(slam_ekf_factor_t* f, int dtype, int max_landmarks, int device, int panel_tiles);

/* Synchronises the factor's stream and frees everything; a null handle is SLAM_OK. */
int slam_ekf_factor_destroy(slam_ekf_factor_t f);

/* L L' = P[0 : n, 0 : n] of src, and a snapshot of x.  SLAM_OK, SLAM_E_NOTPD (info is filled in both cases), or a refusal. */
int slam_ekf_factor_compute(slam_ekf_factor_t f, slam_ekf_t src, double info[8]);

/* info of the last compute (all zero except [2] = -1 and [7] before the first). */
int slam_ekf_factor_info(slam_ekf_factor_t f, double info[8]);

/* out[(c - c0) ld_out + (r - r0)] = L[r, c] for r0 <= r < r0 + nr, c0 <= c < c0 + nc, in the factor's dtype, +0.0 above the
 * diagonal.  SLAM_E_BADARG: negative arguments, r0 + nr > n, c0 + nc > n, ld_out < nr, a null out with nr nc > 0. */
int slam_ekf_factor_get(slam_ekf_factor_t f, int r0, int c0, int nr, int nc, void* out, int ld_out);

/* x[0 : n) as compute found it, converted to double. */
int slam_ekf_factor_mean(slam_ekf_factor_t f, double* x);

/* d2 may be null. */
int slam_ekf_factor_solve(slam_ekf_factor_t f, const double* B, int r, int ldb, double* Y, double* d2);

int slam_ekf_factor_multiply(slam_ekf_factor_t f, const double* Z, int r, int ldz, double* out);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_FACTOR_H */
