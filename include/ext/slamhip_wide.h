/* slamhip_wide.h -- the joint update of up to 64 range-bearing observations in ONE down-date, its Jacobians evaluated where the caller
 * says: at the linearisation points of a first-estimates object (slamhip_fej.h) or at the stored state.  The entry points of the
 * EXTENSION library libslamhip_wide.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare, and libslamhip_fej.so exactly what slamhip_fej.h declares.  libslamhip_wide.so is built from csrc/ekf_wide.hip by the same
 * Makefile, links against libslamhip.so only (it works on that library's handles, borrows their update workspace and ends an update
 * in that library's down-date) and is found beside it.  It READS a first-estimates object (its handle, its count, lin and first) and
 * calls nothing of libslamhip_fej.so.  Same conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the
 * message.
 *
 * WHY.  slam_ekf_fej_update takes 8 observations, the width of the 16 x 16 front half it shares with its siblings.  A step's 58
 * matched observations then go as 8 sequential updates, 8 passes over P, and the chain is not the joint update: the residuals of batch
 * b are taken at the mean batch b - 1 left.  This library is the wide front half: k = 2m <= 128 rows, one pass over P.
 *
 * THE RULE (tests/wide_ref.py runs it literally in float64).  All arithmetic up to the rounding of a stored entry is in double
 * whatever the state's dtype; x and P are the stored (rounded) values.
 *
 * update (h, f, zf, idf, m, R, out[4]), 1 <= m <= SLAM_WIDE_MAXOBS.  zf, idf, R as slam_ekf_fej_update takes them; a landmark named
 *     twice in idf is observed twice.  For every k: zp_k = the observation model at the stored x, v_k = z_k - zp_k with the bearing
 *     wrapped ONCE; Hv_k, Hf_k = the same model's Jacobian blocks (src/common.jl:139-165) evaluated
 *         with f given:   at the pose f's lin and the landmark f's first[idf[k]] (f must belong to h);
 *         with f == NULL: at the stored x -- the product's Cholesky-form update (src/ekf.jl:67-75).
 *     From there on:
 *         S = H P H' + I (x) R, S <- (S + S') / 2, S = L L' right-looking; a pivot <= 0 or not finite FAILS
 *         C = inv(chol(S)) (upper), g = C C' v
 *         W1 = P H' C rounded ONCE to the state's dtype, zero-padded to a multiple of 16 columns;  x += P H' g (x[2] is NOT wrapped)
 *         P -= W1 W1' by ONE call of the product library's down-date on the plain panel of round_up(2m, 16) columns
 *     out = { v' inv(S) v, log det S, the smallest l_jj or the failing pivot, -1 or the failing pivot's index }.
 *     SLAM_E_NOTPD leaves x, P and the packed diagonal blocks bit for bit (the status word is set, the panel is written as zero, x is
 *     not touched).  lin and first are never changed.  SYNCHRONISES, like slam_ekf_fej_update.
 *
 * nis: the same arguments; the front half only, the state only read; the same four numbers, bit for bit those the update would
 *     return.  The joint chi-square gate of a whole batch at the linearisation points, before it is committed.
 *
 * limits: out = { SLAM_WIDE_MAXOBS }.  Touches no device.
 *
 * PRECISION.  The front half (the model, S, its factor, C, g, P H', W1 before its one rounding) is in double, so its error is
 * cond(S) u64.  W1 is rounded once to the state's dtype, so the covariance error is the down-date's, as for slam_ekf_update.
 *
 * SLAM_E_BADARG, decided on the host before anything is enqueued: a null handle or pointer; m outside 1 .. 64; an id outside 1 .. N;
 * zf or R not finite, R not symmetric or not positive definite; with f given: f's handle is not h, or f's count differs from h's N
 * ("the map changed outside the object": call slam_ekf_fej_remap).
 */
#ifndef SLAMHIP_WIDE_H
#define SLAMHIP_WIDE_H

#include "slamhip_fej.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_WIDE_MAXOBS 64

int slam_ekf_wide_update(slam_ekf_t h, slam_ekf_fej_t f, const double* zf, const int32_t* idf, int m, const double R[4], double out[4]);

int slam_ekf_wide_nis(slam_ekf_t h, slam_ekf_fej_t f, const double* zf, const int32_t* idf, int m, const double R[4], double out[4]);

int slam_ekf_wide_limits(int32_t out[1]);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_WIDE_H */
