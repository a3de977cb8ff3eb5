/* slamhip_join.h -- map joining (Tardos et al.): a second EKF map appended to this one on the device, the entry point of the
 * COMPANION library libslamhip_join.so.  No counterpart in the reference.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_join.so is built from csrc/ekf_join.hip by the same Makefile, links against libslamhip.so (it works on
 * that library's handles and calls its internal helpers: both come from one tree and one make) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message. */
#ifndef SLAMHIP_JOIN_H
#define SLAMHIP_JOIN_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Join the local map b into the global map a.  b's frame is a's current vehicle pose (x, y, phi): b was started there with pose
 * (0, 0, 0) and zero covariance and a has neither moved nor observed since, so the two are independent.  With c = cos phi,
 * s = sin phi (double, from a's stored heading) a point p of b lies at g(p) = (x + c px - s py, y + s px + c py) with the Jacobian
 * J(p) = [1 0 -(s px + c py); 0 1 c px - s py] against a's pose and R = [c -s; s c] against p itself.
 *   means:  a's vehicle <- (g(b's vehicle position), mpi_to_pi(phi + phi_b)); a's landmarks stay; b's landmark j becomes a's
 *           landmark N_a + j with mean g(b_j).
 *   P:      for b's groups gr, gc (0 the pose pair, 1 the heading, >= 2 a landmark pair; J_g = J(p_g), R_g = R for a pair,
 *           J_g = [0 0 1], R_g = 1 for the heading; groups 0 and 1 land on a's indices 0 .. 2, landmark j at 3 + 2 (N_a + j - 1)):
 *               P'[dest gr, dest gc] = J_gr P_a[0:3, 0:3] J_gc' + R_gr P_b[gr, gc] R_gc'
 *               P'[dest gr, col]     = J_gr P_a[0:3, col]            for an old landmark column col >= 3 of a
 *           a's landmark-landmark part is not written at all.  In dense form P' = F P_a F' + G P_b G'.
 * Every value is computed in double from the stored values of both handles as they were before the call and rounded once to
 * the dtype; an entry and its mirror inside a diagonal tile come from one computed value.
 * first_new (may be NULL) receives the 1-based id in a of b's landmark 1, N_a + 1, also when b has no landmark.
 * Decided before anything is enqueued, both states unchanged bit for bit:
 *   SLAM_E_BADARG    a null handle, a == b, different dtypes, different devices
 *   SLAM_E_CAPACITY  N_a + N_b exceeds a's capacity
 * SLAM_E_HIP from the runtime once work has been enqueued: if a launch failed, a's state is undefined (upload it again); if only
 * the event that orders b behind the join failed, a is joined and consistent, and b must be synchronised with a before it is written.
 * Ordering: b's deferred asynchronous status is resolved first, as slam_ekf_sync(b) would (an error of b is returned, a is
 * untouched).  The work is enqueued on a's stream behind everything enqueued there (a's own deferred status stays pending)
 * and behind an event recorded on b's stream; an event recorded on a's stream after the last read of b is made a dependency of
 * b's stream, so b may be updated, transformed or destroyed as soon as the call returns.  b is never written.  Enqueued, does
 * not synchronise a. */
int slam_ekf_join(slam_ekf_t a, slam_ekf_t b, int32_t* first_new);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_JOIN_H */
