/* slamhip_iterated.h -- the iterated EKF update (IEKF: Gauss-Newton on the MAP cost of one batch of range-bearing observations),
 * relinearised on the device.  The entry points of the EXTENSION library libslamhip_iterated.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_iterated.so is built from csrc/ekf_iterated.hip by the same Makefile, links against libslamhip.so (it works
 * on that library's handles, borrows their update workspace and ends in that library's rank-16 down-date) and is found beside it.
 * Same conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message.  The header lives in
 * include/ext/ and is found through the same -I as the others.
 *
 * WHY.  slam_ekf_update linearises the range-bearing model once, at the prior mean (src/ekf.jl:46-77).  With a wide pose prior and an
 * accurate sensor the mean it returns is not the minimum of the cost the filter claims to minimise,
 *     J(x) = (x - x0)' inv(P) (x - x0) + sum_k r_k(x)' inv(R) r_k(x),        r_k(x) = z_k - h_k(x), bearing wrapped,
 * and the error stays in the map.  The iterated update relinearises at each iterate.  It is Gauss-Newton WITHOUT a line search:
 * descent is not promised, which is what slam_ekf_iterated_nis (the dry run) and out[8], out[9] are for.
 *
 * ARGUMENTS.  zf and idf as slam_ekf_update takes them: m (range, bearing) pairs and m 1-based landmark ids, duplicates allowed.
 * 1 <= m <= SLAM_ITERATED_MAXOBS (16 rows: W1 is the plain 16-column panel of the down-date).  R is 2 x 2, column-major, EXACTLY
 * symmetric and positive definite.  1 <= max_iter <= 64.  tol >= 0 and finite.
 *
 * THE RULE (tests/iterated_ref.py runs it literally in float64).  Everything up to W1 is in double whatever the state's dtype; x0 and
 * P are the stored (rounded) values, P read as the symmetric matrix its stored entries define.  a = (0, 1, 2) followed by the two
 * state indices of every idf[k] in the order given, duplicates kept: 3 + 2m <= 19 indices.  H touches only these states, and their
 * iterates depend on P only through the block P[a, a], so the reduced iteration below IS the full n-dimensional one:
 *     x_0 = x0[a]
 *     for i = 0 .. max_iter - 1:
 *         (zp_k, Hv_k, Hf_k) = the observation model at x_i for every k            (src/common.jl:139-165)
 *         r_k = z_k - zp_k, the bearing wrapped ONCE (mpi_to_pi);   v_i = r - H_i (x0[a] - x_i)            (i = 0: v_0 = r)
 *         S_i = H_i P[a, a] H_i' + I_m (x) R,   S <- (S + S') / 2,   S = L L' right-looking; a pivot <= 0 or not finite FAILS
 *         g_i = inv(S_i) v_i;     x_{i+1} = x0[a] + P[a, a] H_i' g_i
 *         step_i = max |x_{i+1} - x_i|;   stop after this iteration when step_i <= tol
 *     commit with the LAST H_i, C_i = inv(chol(S_i)) (upper) and g_i:
 *         PHt = P H_i' (all n rows),   W1 = PHt C_i rounded ONCE to the state's dtype, zero-padded to 16 columns
 *         x  += PHt g_i                each entry rounded once; x[2] is NOT wrapped, as slam_ekf_update leaves it (src/ekf.jl:74)
 *         P  -= W1 W1'                 the product library's down-date of a plain 16-column panel
 * With max_iter = 1 this is the reference's Cholesky-form update.
 *
 * out[10], double (out may NOT be null):
 *     [0] the iterations run                           [1] 1 if the last step was <= tol, else 0
 *     [2] the last step                                [3] v' inv(S) v of the last iteration
 *     [4] log det S of the last iteration              [5] the smallest l_jj of the last iteration, or the failing pivot
 *     [6] -1, or the failing pivot's index             [7] -1, or the failing iteration
 *     [8] J(x_1)                                       [9] J(x_last)
 * J(x_{i+1}) = g_i' (S_i - I (x) R) g_i + sum_k r_k(x_{i+1})' inv(R) r_k(x_{i+1}): the MAP cost at the iterate; the first term is the
 * prior's, since x_{i+1} - x0 = P H_i' g_i.  After a failure at iteration i: [0] = i (the iterations completed), [1] = 0, [2], [8] and
 * [9] of the last completed iteration (0 when i = 0), [3] = [4] = 0.
 *
 * NOT POSITIVE DEFINITE at any iteration: the call returns SLAM_E_NOTPD with out filled, and x, P and the packed diagonal blocks are
 * bit for bit what they were: the panel kernel writes a zero panel and leaves x alone when the status word is set, and the down-date
 * returns at once on the same word.
 *
 * SLAM_E_BADARG, decided on the host before anything is enqueued: a null handle or pointer; m outside 1 .. SLAM_ITERATED_MAXOBS;
 * max_iter outside 1 .. 64; tol negative or not finite; an id outside 1 .. N; a zf or R that is not finite; R not symmetric or not
 * positive definite.
 *
 * SYNCHRONISES, like slam_ekf_update_linear: the call reads out and its status word back before it returns.  Afterwards the packed
 * diagonal blocks agree with the matrix (the down-date keeps them) and the grid form of the gating is rebuilt at the next query,
 * since the means moved.
 *
 * slam_ekf_iterated_nis runs the same iteration under the same argument rules and fills the same out; x and P are only read.  The
 * dry run a caller uses to decide whether to commit.  SLAM_E_NOTPD as above.  Synchronises.
 *
 * slam_ekf_iterated_limits: out = {SLAM_ITERATED_MAXOBS, 64}.
 */
#ifndef SLAMHIP_ITERATED_H
#define SLAMHIP_ITERATED_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_ITERATED_MAXOBS 8
#define SLAM_ITERATED_MAXITER 64

int slam_ekf_update_iterated(slam_ekf_t h, const double* zf, const int32_t* idf, int m, const double R[4], int max_iter, double tol,
                             double out[10]);

int slam_ekf_iterated_nis(slam_ekf_t h, const double* zf, const int32_t* idf, int m, const double R[4], int max_iter, double tol,
                          double out[10]);

int slam_ekf_iterated_limits(int32_t out[2]);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_ITERATED_H */
