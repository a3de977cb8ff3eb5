/* slamhip_fej.h -- first-estimates Jacobian (FEJ) predict, update and augment for the EKF, the linearisation points kept on the
 * device beside the state.  The entry points of the EXTENSION library libslamhip_fej.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_fej.so is built from csrc/ekf_fej.hip by the same Makefile, links against libslamhip.so (it works on that
 * library's handles, borrows their update workspace and ends an update in that library's rank-16 down-date) and is found beside it.
 * Same conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message.
 *
 * WHY.  2-D range-bearing SLAM has three unobservable directions: the two translations and the rotation of the whole map.  The
 * standard EKF evaluates every Jacobian at the newest estimate; the rotation then looks observable, the filter gains information
 * that does not exist, and the heading variance with everything correlated to it shrinks too fast (Huang, Mourikis and Roumeliotis,
 * "Observability-based rules for designing consistent EKF SLAM estimators", IJRR 2010; Bailey et al. 2006).  The remedy changes no
 * formula, only where the Jacobians are evaluated: every landmark at its FIRST estimate, the vehicle at its PREDICTED pose, never
 * at an updated one.
 *
 * THE OBJECT.  slam_ekf_fej_t f is attached to an EKF handle h (which must outlive it) and holds on the device, as doubles:
 * lin[3], the vehicle's linearisation pose, and first[2 maxN], every landmark's first estimate; and its own landmark count.
 *
 * THE RULE (tests/fej_ref.py runs it literally in float64).  J = [0 -1; 1 0].  All arithmetic up to the rounding of a stored entry
 * is in double whatever the state's dtype; x and P are the stored (rounded) values.
 *
 * create.   lin <- the stored pose, first <- the stored landmark means, the count is h's N.
 *
 * predict (v, g, wheelbase, Q, dt).  The new pose x+ by the reference's formulas (src/ekf.jl:38-41) from the stored pose, each entry
 *     rounded to the state's dtype (x+ as stored); Gu the reference's, at the stored heading; Gv = I3 with its third column's top two
 *     entries set to J (x+[0:2] - lin[0:2]).  P_vv <- Gv P_vv Gv' + Gu Q Gu', P_v,rest <- Gv P_v,rest and its mirror.  Then
 *     lin <- x+.  Enqueued; does not synchronise.
 *
 * update (zf, idf, m <= SLAM_FEJ_MAXOBS, R, out[4]).  zf, idf, R as slam_ekf_update_iterated takes them; duplicate ids allowed.
 *     For every k: zp_k = the observation model at the stored x, r_k = z_k - zp_k with the bearing wrapped ONCE; Hv_k, Hf_k = the same
 *     model's Jacobian blocks (src/common.jl:139-165) evaluated at the pose lin and the landmark first[idf[k]].  From there the
 *     reference's Cholesky form (src/ekf.jl:67-75) exactly as slamhip_iterated.h states it for one iteration:
 *         S = H P H' + I (x) R, S <- (S + S') / 2, S = L L' right-looking; a pivot <= 0 or not finite FAILS
 *         W1 = P H' C rounded ONCE to the state's dtype, zero-padded to 16 columns;  x += P H' g (x[2] is NOT wrapped)
 *         P -= W1 W1' by the product library's down-date of a plain 16-column panel
 *     out = { v' inv(S) v, log det S, the smallest l_jj or the failing pivot, -1 or the failing pivot's index }.
 *     SLAM_E_NOTPD leaves x, P and the packed diagonal blocks bit for bit (a lin that coincides with a first estimate ends here too:
 *     the Jacobian, and with it the first pivot, is not finite).  lin and first are not changed.  SYNCHRONISES, like
 *     slam_ekf_update_linear and slam_ekf_update_iterated.
 *
 * augment (zn, cnt, R).  For each new observation in turn: the mean lm and Gz are the reference's (src/ekf.jl:94-103) from the stored
 *     pose; Gv = [I2 | J (lm - lin[0:2])] with lm the mean AS STORED; the new rows and the diagonal block by src/ekf.jl:112-118 with
 *     this Gv; first of the new landmark <- lm.  Keeps the packed diagonal blocks.  Capacity as in slam_ekf_augment
 *     (SLAM_E_CAPACITY, decided before anything is enqueued).  Both counts grow by cnt.
 *
 * reset (ids, cnt, pose).  first of the listed landmarks (1-based, 1 .. N) <- their stored means; cnt = -1: all of them (ids may be
 *     null).  pose != 0: lin <- the stored pose as well.
 *
 * remap (ids, cnt).  After the map was renumbered OUTSIDE the object (slam_ekf_remove_landmarks, _merge_landmarks, _select, _join):
 *     cnt must equal h's N; new landmark j takes the first estimate of old landmark ids[j] (1-based, at most the object's old count),
 *     ids[j] = 0 takes the current stored mean.  The object's count becomes cnt.
 *
 * transform (tx, ty, theta).  The map slamhip_frame.h states for the means, applied to lin and every first estimate; lin's heading is
 *     wrapped once.  Call it beside slam_ekf_transform.
 *
 * get / set (lin[3], first[2 N], count).  The three as doubles, to and from the host (null: not wanted / left as it is): for
 *     checkpoints and designed tests.  set: first holds 2 h->N values and the count becomes h's N.  Both synchronise.
 *
 * limits: out = { SLAM_FEJ_MAXOBS }.
 *
 * WHY THIS PRESERVES THE THREE DIRECTIONS.  Let N have the vehicle rows [I2 | J lin_xy; 0 0 1] and the landmark rows
 * [I2 | J first_j].  Then H N = 0 for every update, Gv of predict maps the old N's vehicle rows to the new N's, and Gv of augment
 * produces the new landmark's rows: N' inv(P) N, the information along the three directions, never grows.
 *
 * SLAM_E_BADARG, decided on the host before anything is enqueued: a null handle, object or pointer; predict, update, augment, reset
 * and transform when the object's count differs from h's N ("the map changed outside the object"); for update every argument rule of
 * slam_ekf_update_iterated (m outside 1 .. 8, an id outside 1 .. N, zf or R not finite, R not symmetric or not positive definite); a
 * value of predict or transform that is not finite; cnt < 0 or an R as before for augment; an id outside its range for reset and
 * remap.
 */
#ifndef SLAMHIP_FEJ_H
#define SLAMHIP_FEJ_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_FEJ_MAXOBS 8

typedef struct slam_ekf_fej* slam_ekf_fej_t;

int slam_ekf_fej_create(slam_ekf_fej_t* f, slam_ekf_t h);

int slam_ekf_fej_destroy(slam_ekf_fej_t f);

int slam_ekf_fej_predict(slam_ekf_fej_t f, double v, double g, double wheelbase, const double Q[4], double dt);

int slam_ekf_fej_update(slam_ekf_fej_t f, const double* zf, const int32_t* idf, int m, const double R[4], double out[4]);

int slam_ekf_fej_augment(slam_ekf_fej_t f, const double* zn, int cnt, const double R[4]);

int slam_ekf_fej_reset(slam_ekf_fej_t f, const int32_t* ids, int cnt, int pose);

int slam_ekf_fej_remap(slam_ekf_fej_t f, const int32_t* ids, int cnt);

int slam_ekf_fej_transform(slam_ekf_fej_t f, double tx, double ty, double theta);

int slam_ekf_fej_get(slam_ekf_fej_t f, double lin[3], double* first, int32_t* count);

int slam_ekf_fej_set(slam_ekf_fej_t f, const double lin[3], const double* first);

int slam_ekf_fej_limits(int32_t out[1]);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_FEJ_H */
