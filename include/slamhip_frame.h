/* slamhip_frame.h -- the rigid frame change of both filters (the map re-anchored: a surveyed site frame, a GPS datum, another
 * vehicle's frame), entry points of the COMPANION library libslamhip_frame.so.  No counterpart in the reference.
 *
 * Why a library of its own: what libslamhip.so exports is exactly what slamhip.h (the drop-in boundary, at most 60 entry points)
 * and slamhip_diag.h (22 measurement / read-out / map-management hooks) declare, and the tests hold both headers to those
 * counts.  libslamhip_frame.so is built from csrc/ekf_transform.hip and csrc/pf_transform.hip by the same Makefile, links
 * against libslamhip.so (it works on that library's handles and calls its internal helpers: a link-time contract, both
 * libraries come from one tree and one make; never pass it the handles of another build of libslamhip) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message. */
#ifndef SLAMHIP_FRAME_H
#define SLAMHIP_FRAME_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The whole state expressed in another frame: every position (the vehicle's and every landmark mean) p <- R p + t with
 * R = [c -s; s c], the heading phi <- mpi_to_pi(phi + theta) (the reference's single wrap), P <- T P T' with
 * T = blockdiag(R, 1, R, R, ...).  theta is reduced with remainder(theta, 2 pi); c = cos, s = sin are evaluated once on the host in
 * double, there is no device trigonometry.  Every 2 x 2 block B of P with rows (r0, r0 + 1) and columns (c0, c0 + 1) of the state
 * pairs (0,1), (3,4), (5,6), ... becomes R B R', evaluated in double from the stored values and rounded once to the handle's
 * dtype; row and column 2 are rotated from the other side only; P[2, 2] is unchanged bit for bit.  One in-place pass over the
 * stored tiles; c == 1 and s == 0 (a pure translation) leaves P alone, bit for bit.
 * SLAM_E_BADARG (state unchanged): null handle, a non-finite argument.
 * Ordered on the handle's stream behind everything enqueued before it (async updates included, whose deferred status stays
 * pending for slam_ekf_sync); enqueued, does not synchronise. */
int slam_ekf_transform(slam_ekf_t h, double tx, double ty, double theta);

/* ---- FastSLAM: the filter expressed in another frame ------------------------------------------------------------------------
 * Every particle's pose as slam_ekf_transform moves the vehicle's (heading: wrap_pi(phi + theta) in the filter's dtype) and every
 * landmark record IN USE (the rule of the read-outs in slamhip_diag.h: Pxx > 0, or Pxx == 0 with the landmark `seen`):
 *   m <- R m + t,   Pxx' = c^2 Pxx - 2cs Pxy + s^2 Pyy,   Pxy' = cs (Pxx - Pyy) + (c^2 - s^2) Pxy,   Pyy' = s^2 Pxx + 2cs Pxy + c^2 Pyy,
 * evaluated in double and rounded once.  An empty slot (Pxx = -1) and a never-seen all-zero record stay as they are bit for bit.
 * Pxx is the in-use mark: a record that had Pxx > 0 and whose rounded Pxx' is not > 0 receives the smallest positive normal
 * number of the dtype.  The log-weights (beyond a pending normalisation shift, honoured as slam_pf_download honours it), the RNG
 * step, `seen` and the resampling count are untouched.  Leaves the auto mode, materialises lazily resampled maps, is collective
 * while peers are attached (all as slam_pf_step_unknown); enqueued.
 * SLAM_E_BADARG (state unchanged): null handle, a non-finite argument. */
int slam_pf_transform(slam_pf_t h, double tx, double ty, double theta);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_FRAME_H */
