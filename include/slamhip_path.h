/* slamhip_path.h -- per-particle trajectory history for FastSLAM: a ring of pose snapshots and ancestor arrays kept on the device,
 * and the read-outs that follow the CURRENT particles back through it (the path of one particle, of the best one, the weighted
 * mean path, and the number of distinct ancestors still alive k records back), the entry points of the COMPANION library
 * libslamhip_path.so.  No counterpart in the reference.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_path.so is built from csrc/pf_path.hip by the same Makefile, links against libslamhip.so (it works on that
 * library's handles and calls its internal helpers: both come from one tree and one make) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message, state unchanged on
 * SLAM_E_BADARG.
 *
 * Why: each particle is a hypothesis about the WHOLE vehicle path, but slam_pf_get_mean_pose and slam_pf_get_particle give the
 * current pose only, and every resampling permutes the poses and overwrites the ancestors of the one before.  The path object
 * is the missing record.  It BORROWS the filter handle (destroy it before the filter) and holds a ring of `cap` slots, each
 *   - a snapshot of the poses, [3][n] in the filter's dtype;
 *   - an ancestor array, [n] int32: anc[p] is the index, AT THE PREVIOUS RECORD, of the particle that p descends from;
 *   - a flag: the ancestor array is in use (a resampling went through this object since the previous record), or the slot's
 *     ancestors are the identity and the array is not read;
 * two "pending" ancestor buffers [n] int32 for the resamplings since the last record (their composition is out of place), and a
 * few hundred bytes of flags and counters.
 * MEMORY: cap * (3 * esz + 4) * n + 8 n bytes of device memory (esz = 4 or 8: 4 MB per slot at 262144 fp32 particles).  The
 * read-outs use a grow-only scratch of their own, allocated at the first one: slam_pf_path_mean (L + 1) * ceil(n / 64) * 32
 * bytes (33 MB at 262144 particles and L = 256), slam_pf_path_survivors 2 n bytes, slam_pf_path_trace cnt * (8 + 24 L) bytes.
 *
 * THE RULE (tests/path_ref.py runs it literally):
 *   record     the live poses go into the next slot (the oldest one when the ring is full) with the composed pending map, or
 *              flagged "identity" when nothing is pending; nothing is pending afterwards.
 *   resample   slam_pf_resample_local, then pend'[p] = pend[anc[p]], or anc[p] when nothing was pending, with the ancestors anc
 *              that call formed (an ancestor outside 0 .. n - 1 -- the library writes none -- counts as p).
 *   trace      a current particle p sits, at the newest record, at index pend[p] (p when nothing is pending); one record
 *              further back at that slot's anc[index] (or the same index: identity).  L = min(records made, cap) are held.
 *
 * SHARDED FILTERS ARE OUT OF SCOPE: only a filter that lives wholly on one shard (n == n_global) with no peers attached is
 * supported.  slam_pf_path_create refuses anything else with SLAM_E_BADARG, and so does every later call once peers have been
 * attached to the filter.
 *
 * RESAMPLING: a filter that has a path object is resampled through slam_pf_path_resample ONLY.  Any other resampling
 * (slam_pf_resample_local, slam_pf_resample_apply, slam_pf_resample, the auto mode's device-side resampling) moves the particles
 * and leaves the pending map where it was: the history no longer belongs to the particles.  A filter that has BOTH a path
 * object and an evidence object (slamhip_evidence.h) cannot be resampled through both: that combination is out of scope.
 *
 * The read-outs (get, trace, best, mean, survivors) leave the poses, the log-weights, the landmark records, the RNG step and
 * the ring unchanged bit for bit; like slam_pf_get_map they leave the auto mode first.  With no record made yet (L == 0) each of
 * these five is SLAM_E_BADARG. */
#ifndef SLAMHIP_PATH_H
#define SLAMHIP_PATH_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_PF_PATH_MAXTRACE 4096

typedef struct slam_pf_path* slam_pf_path_t;

/* A path object of `cap` slots for filter h; no record yet.  SLAM_E_BADARG: a null argument, cap < 1, a shard of a larger
 * filter, peers attached. */
int slam_pf_path_create(slam_pf_path_t* ph, slam_pf_t h, int cap);
/* Waits for the handle's stream, frees the buffers.  The filter is not touched.  A null ph is SLAM_E_BADARG. */
int slam_pf_path_destroy(slam_pf_path_t ph);

/* One record (see THE RULE): one launch that copies 3 n values, and n int32 more when a resampling is pending.  Begins as
 * slam_pf_transform does (leaves the auto mode); the landmark records are not materialised: only poses are read.  Enqueued on
 * the handle's stream, no host synchronisation. */
int slam_pf_path_record(slam_pf_path_t ph);

/* slam_pf_resample_local(h, gmax, u0), then on the same stream the pending map is composed with the ancestors that call formed.
 * The filter is exactly what slam_pf_resample_local leaves; a status of that call is returned as it is, with the pending map
 * unchanged.  Enqueued. */
int slam_pf_path_resample(slam_pf_path_t ph, double gmax, double u0);

/* out = {L, records ever made, cap, resamplings seen}.  Host only. */
int slam_pf_path_info(slam_pf_path_t ph, int64_t out[4]);

/* The record k back (k = 0: the newest; 0 <= k < L): pose [3][n] widened to double, anc [n] (the identity 0 .. n - 1 when the
 * slot is flagged "identity"), *has_anc 1 or 0.  Each of the three may be NULL.  Synchronises. */
int slam_pf_path_get(slam_pf_path_t ph, int k, double* pose, int32_t* anc, int* has_anc);

/* The paths of the CURRENT particles ids[0 .. cnt) (0 <= id < n, 1 <= cnt <= SLAM_PF_PATH_MAXTRACE): out[c][t][3] = (x, y, phi)
 * of the ancestor of ids[c] at record t, t = 0 the oldest held record ... L - 1 the newest.  The values are the stored ones
 * widened to double, exact.  One thread per requested particle walks the slots.  Synchronises. */
int slam_pf_path_trace(slam_pf_path_t ph, const int64_t* ids, int cnt, double* out);

/* The path of the particle slam_pf_get_particle(h, -1, ...) names: the largest log-weight as slam_pf_download shows it (a
 * normalisation shift that slam_pf_normalize deferred is applied in the storage type; with none deferred: the stored value),
 * the lowest index on a tie, a NaN never wins (every log-weight NaN: particle 0).  Found on the device, then traced:
 * out[L][3]; *idx (may be NULL) the particle.  Synchronises. */
int slam_pf_path_best(slam_pf_path_t ph, int64_t* idx, double* out);

/* The mean path under the CURRENT weights: out[t] = {x, y, phi, R}, t as in slam_pf_path_trace, the mean over ALL current
 * particles p of their ancestors' poses at record t with w_p = exp((double)logw_p - max logw) from the stored log-weights (a
 * deferred normalisation shift is a constant and cancels): x = sum w x / sum w, y likewise, phi = atan2(sum w sin phi,
 * sum w cos phi), R = hypot(sum w sin phi, sum w cos phi) / sum w, the mean resultant length of the headings (1: all equal).
 * The sums are formed in double on the device over a FIXED tree (inside each wave of 64 consecutive particles, then over the
 * waves in a fixed order; no floating-point atomics): two calls give the same bits.  Synchronises. */
int slam_pf_path_mean(slam_pf_path_t ph, double* out);

/* out[t] (t as above, L values): the number of distinct particles at record t that have a descendant among the current
 * particles.  out[L - 1] <= n, non-increasing going back; n at every record when no resampling went through the object.  The
 * standard depletion diagnostic.  Exact integers.  Synchronises. */
int slam_pf_path_survivors(slam_pf_path_t ph, int64_t* out);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_PATH_H */
