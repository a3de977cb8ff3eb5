/* slamhip_evidence.h -- landmark evidence for FastSLAM with unknown correspondences: one existence counter per landmark slot and
 * particle, kept on the device, and the pruning of landmarks whose counter falls below zero (Probabilistic Robotics, Table 13.1;
 * Montemerlo's thesis), the entry points of the COMPANION library libslamhip_evidence.so.  No counterpart in the reference.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_evidence.so is built from csrc/pf_evidence.hip by the same Makefile, links against libslamhip.so (it works
 * on that library's handles and calls its internal helpers: both come from one tree and one make) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message, state unchanged on
 * SLAM_E_BADARG.
 *
 * Why: slam_pf_update_unknown / slam_pf_step_unknown start a landmark in the particle's lowest unused slot for every observation
 * that no slot explains, and nothing ever removes one: one false detection per step fills a particle's map for good.  The evidence
 * object is the missing half.  It BORROWS the filter handle (destroy it before the filter) and holds
 *   - one int8 counter per (slot, particle), [nl][n] with the particle index fastest, in two buffers (the resampling gather is out
 *     of place); SLAM_PF_EVIDENCE_EMPTY = -128 means "no landmark here", a live counter is 0 .. cap, cap <= 127;
 *   - a device buffer [64][n] int32 for the decisions of slam_pf_step_unknown_evidence.
 *
 * SHARDED FILTERS ARE OUT OF SCOPE: only a filter that lives wholly on one shard (n == n_global) with no peers attached is
 * supported.  slam_pf_evidence_create refuses anything else with SLAM_E_BADARG, and so does every later call once peers have been
 * attached to the filter.
 *
 * RESAMPLING: a filter that has an evidence object is resampled through slam_pf_evidence_resample ONLY.  Any other resampling
 * (slam_pf_resample_local, slam_pf_resample_apply, slam_pf_resample, the auto mode's device-side resampling) moves the particles
 * and leaves the counters where they were: they no longer belong to their particles. */
#ifndef SLAMHIP_EVIDENCE_H
#define SLAMHIP_EVIDENCE_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_PF_EVIDENCE_EMPTY (-128)
#define SLAM_PF_EVIDENCE_MAXOBS 64

typedef struct slam_pf_evidence* slam_pf_evidence_t;

/* An evidence object for filter h; every counter starts at SLAM_PF_EVIDENCE_EMPTY (records the filter already holds receive
 * `init` at the first update).  SLAM_E_BADARG: a null argument, a shard of a larger filter, peers attached. */
int slam_pf_evidence_create(slam_pf_evidence_t* ev, slam_pf_t h);
/* Waits for the handle's stream, frees the buffers.  The filter is not touched.  A null ev is SLAM_E_BADARG. */
int slam_pf_evidence_destroy(slam_pf_evidence_t ev);

/* One pass of the rule over the records of the filter and the particles' current poses.  d_assoc: the DEVICE array [m][n] int32
 * that slam_pf_update_unknown / slam_pf_step_unknown wrote for the call just made (slot >= 0 matched, negative: not); the
 * caller's buffer, 16-byte aligned for the fastest path.  The kernel only ever COMPARES these values, it indexes nothing with them.
 *
 * Each (particle p, slot l) independently, the first case that applies, with used = !(Pxx < 0) (the in-use test of the
 * association) and c the counter:
 *   1. !used:                      c <- EMPTY.  (slam_pf_clear_landmarks from outside is followed without a hook.)
 *   2. used and c == EMPTY:        c <- init.   The record was created since the last pass -- by this step's new-landmark branch
 *                                  or by slam_pf_init_landmarks; read from the record, not from d_assoc (an assoc of -1 that found no
 *                                  slot created nothing).
 *   3. used, some i < m has d_assoc[i][p] == l:   c <- min(c + inc, cap), once per call however many observations matched.
 *   4. used, unmatched, in view:   c <- c - dec; below 0 the record becomes the empty record (0, 0, -1, 0, 0) of
 *                                  slam_pf_clear_landmarks and c <- EMPTY.
 *   5. otherwise unchanged.
 * In view, in the filter's dtype T from the stored values with the plain functions of the association:
 *   dx = lx - x, dy = ly - y, d = sqrt(dx dx + dy dy), b = wrap_pi(atan2(dy, dx) - phi);  d <= (T)r_max && fabs(b) <= (T)half_fov.
 *
 * counts (may be NULL; otherwise the call synchronises) receives, totalled over all particles and slots:
 *   {records in use after the call, created (case 2), decremented (case 4, the pruned ones included), pruned}.
 * Begins as slam_pf_transform does (leaves the auto mode, materialises lazily resampled maps); enqueued on the handle's stream.
 * Neither a pose, a log-weight nor the RNG step is touched.
 * SLAM_E_BADARG (nothing changed): null ev; m outside 0 .. 64; d_assoc NULL with m > 0; r_max not finite or <= 0; half_fov outside
 * (0, pi]; inc < 1; dec < 1; not 0 <= init <= cap <= 127; peers attached to the filter since create. */
int slam_pf_evidence_update(slam_pf_evidence_t ev, const int32_t* d_assoc, int m, double r_max, double half_fov, int inc, int dec,
                            int init, int cap, int64_t counts[4]);

/* The call a user makes per step: slam_pf_step_unknown(h, V, ..., gate2, <the object's own decision buffer>, out) followed by
 * slam_pf_evidence_update with those decisions.  out[3] is slam_pf_step_unknown's (pruning touches no weight); counts as above
 * (may be NULL).  Every argument of both calls is checked before anything is enqueued. */
int slam_pf_step_unknown_evidence(slam_pf_evidence_t ev, double V, double G, double wheelbase, const double Q[4], double dt,
                                  const double* z, int m, const double R[4], double gate1, double gate2, double r_max,
                                  double half_fov, int inc, int dec, int init, int cap, double out[3], int64_t counts[4]);

/* slam_pf_resample_local(h, gmax, u0), then on the same stream the counters follow their particles: c'[l][p] = c[l][anc[p]] with
 * the ancestors that call formed.  The filter is exactly what slam_pf_resample_local leaves.  Enqueued. */
int slam_pf_evidence_resample(slam_pf_evidence_t ev, double gmax, double u0);

/* The counters to a host array [nl][n] of int8; synchronises. */
int slam_pf_evidence_get(slam_pf_evidence_t ev, int8_t* out);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_EVIDENCE_H */
