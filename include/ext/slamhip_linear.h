/* slamhip_linear.h -- caller-supplied motion and measurement models for the EKF on the device: an update from a sparse linear
 * measurement H x = z + noise, its chi-square gate, a predict from a caller's vehicle Jacobian, and a predict from an odometry
 * increment.  The entry points of the EXTENSION library libslamhip_linear.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_linear.so is built from csrc/ekf_linear.hip by the same Makefile, links against libslamhip.so (it works on
 * that library's handles, borrows their update workspace and ends in that library's rank-16 down-date: both come from one tree
 * and one make) and is found beside it.  Same conventions: extern "C", int status codes, slam_last_error() of libslamhip.so
 * carries the message.  The header lives in include/ext/ and is found through the same -I as the others.
 *
 * STATE INDICES in this interface are 0-based: 0, 1, 2 are the vehicle's x, y, phi; landmark j (1-based, as idf) sits at
 * 3 + 2 (j - 1) and the index after it.  n = 3 + 2 N.
 *
 * THE MEASUREMENT is k rows, 1 <= k <= SLAM_LINEAR_MAXROWS, in CSR: row i has the non-zeros ptr[i] .. ptr[i + 1] - 1 of idx / val,
 * ptr[0] = 0, every row 1 .. SLAM_LINEAR_MAXNNZ of them, idx in [0, n) and distinct inside a row (any order), val finite.
 * z has k entries, finite.  R is k x k, column-major with leading dimension k, EXACTLY symmetric, finite, diagonal >= 0; R = 0
 * is allowed (a hard constraint): whether S is positive definite as computed decides.
 *   mode = SLAM_LINEAR_MEASURED (0)    z is the measured value, v = z - H x, (H x)_i summed over the row's non-zeros in the order
 *                                      given; v_i <- mpi_to_pi(v_i) (ONE conditional wrap, src/common.jl:102-110) when bit i of
 *                                      wrap_mask is set (a compass).  Bits >= k must be 0.
 *   mode = SLAM_LINEAR_INNOVATION (1)  z IS the innovation v (the caller linearised a model of their own; H is its Jacobian).
 *                                      wrap_mask must be 0.
 *
 * THE RULE is the reference's Cholesky-form update (src/ekf.jl:67-75) with this H, everything up to W1 in double whatever the
 * state's dtype (tests/linear_ref.py runs it literally):
 *     PHt = P H'                 P read as the symmetric matrix its stored entries define
 *     S   = H PHt + R,   S <- (S + S') / 2
 *     S   = L L'                 right-looking, row by row pivots d_j; d_j <= 0 or not finite: column j FAILS
 *     C   = inv(L)'              (the reference's inv(chol(S)), upper)
 *     W1  = PHt C                rounded ONCE to the state's dtype, padded with zero columns to 16
 *     x  += PHt (C (C' v))       each entry rounded once to the state's dtype
 *     P  -= W1 W1'               the product library's down-date of a plain 16-column panel, the kernel that slam_ekf_update
 *                                runs for up to 8 observations and slam_ekf_merge_landmarks for its pairs
 * The heading is treated exactly as slam_ekf_update treats it: x[2] is NOT wrapped after the update (src/ekf.jl:74).
 *
 * out[4], double (out may NOT be null):
 *     [0] v' inv(S) v = |C' v|^2        [1] log det S = 2 sum_j log l_jj
 *     [2] the smallest l_jj of chol(S); after a failure the failing pivot d_j itself
 *     [3] -1, or the index j of the failing pivot; then [0] = [1] = 0
 *
 * NOT POSITIVE DEFINITE: the call returns SLAM_E_NOTPD with out filled, and x and P are bit for bit what they were: the panel
 * kernel writes a zero panel and leaves x alone when the status word is set, and the down-date returns at once on the same word.
 *
 * SYNCHRONISES, like slam_ekf_merge_landmarks: the call reads out and its own status word back before it returns.  In async
 * mode the sticky status of an earlier asynchronous update is left for slam_ekf_sync, as that call leaves it.
 * AFTERWARDS the packed diagonal blocks (slam_ekf_get_landmark_blocks) agree with the matrix: the down-date keeps them.  The
 * grid form of the gating is rebuilt at the next query, since the means moved; the pre-gate's variance bound stays valid, since
 * variances only shrink.
 *
 * SLAM_E_BADARG, decided on the host before anything is enqueued: a null handle or pointer; k outside 1 .. 16; an unknown mode;
 * mode 1 with a non-zero wrap_mask; mask bits >= k; ptr[0] != 0; a row with 0 or more than 8 non-zeros; an index outside
 * [0, n) or twice in a row; a val, z or R that is not finite; R not symmetric or with a negative diagonal.
 *
 * slam_ekf_linear_nis runs the factor stage only, under the same argument rules, and fills the same out: the chi-square gate a
 * caller applies BEFORE committing a fix.  x and P are only read.  SLAM_E_NOTPD as above.  Synchronises.
 *
 * THE PREDICTS touch the vehicle's three columns of P only, in one launch, arithmetic in double, each stored entry rounded once:
 *     x[0 : 3]  = xv'
 *     P_vv      = Gv P_vv Gv' + Qv        the lower triangle formed once and mirrored; of Qv only the lower triangle is read
 *     P[f, 0:3] = P[f, 0:3] Gv'  f >= 3   (P_vm = Gv P_vm, its mirror wherever the block-lower storage holds one)
 * Everything else of x and P stays bit for bit.  They are enqueued on the state's stream and do NOT synchronise, like
 * slam_ekf_predict, and like it they leave the gating state alone (no landmark mean or variance changes).
 *   predict_linear    xv' = xv, Gv (general 3 x 3) and Qv (symmetric 3 x 3) from the caller, column-major, finite.
 *   predict_odometry  composes the pose with a vehicle-frame increment d = (dx, dy, dtheta) of covariance Q3 (3 x 3 symmetric,
 *                     column-major, only its lower triangle is read), wholly on the device with no read-back of the pose:
 *                     phi = x[2] is read there, s = sin(phi), c = cos(phi) in double,
 *                         xv' = (x + c dx - s dy,  y + s dx + c dy,  mpi_to_pi(phi + dtheta))
 *                         Gv  = [1 0 -(s dx + c dy); 0 1 (c dx - s dy); 0 0 1]
 *                         Gu  = blockdiag([c -s; s c], 1),     Qv = Gu Q3 Gu'  (lower triangle)
 * SLAM_E_BADARG: a null handle or pointer, a value that is not finite.
 */
#ifndef SLAMHIP_LINEAR_H
#define SLAMHIP_LINEAR_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_LINEAR_MAXROWS 16
#define SLAM_LINEAR_MAXNNZ 8
#define SLAM_LINEAR_MEASURED 0
#define SLAM_LINEAR_INNOVATION 1

int slam_ekf_update_linear(slam_ekf_t h, int k, const int32_t* ptr, const int32_t* idx, const double* val, const double* z,
                           const double* R, int mode, uint32_t wrap_mask, double* out);

int slam_ekf_linear_nis(slam_ekf_t h, int k, const int32_t* ptr, const int32_t* idx, const double* val, const double* z,
                        const double* R, int mode, uint32_t wrap_mask, double* out);

int slam_ekf_predict_linear(slam_ekf_t h, const double* xv, const double* Gv, const double* Qv);

int slam_ekf_predict_odometry(slam_ekf_t h, const double* d, const double* Q3);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_LINEAR_H */
