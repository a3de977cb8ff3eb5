/* slamhip_diag.h -- the MEASUREMENT and introspection entry points of libslamhip.so: event timing of the kernels, phase
 * stamps, the copy floor of the down-date, which form of the gating ran, what the exchange between the ranks of a sharded
 * filter saw, the read-outs of the particle filter's state (its map, one particle), its fused unknown-correspondence step and the EKF's map management (landmark removal, duplicate search and merge) that
 * the reference has no counterpart for.  Nothing here is part of the drop-in boundary (include/slamhip.h: what the reference's module surface maps
 * onto); bench.py, the tests and the profiling tools use them.  Same conventions: extern "C", int status codes. */
#ifndef SLAMHIP_DIAG_H
#define SLAMHIP_DIAG_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The diagonal of P (n values, handle dtype) -- a read-out for checks; slam_ekf_get_block / slam_ekf_get_landmark_blocks are the API. */
int slam_ekf_get_diag(slam_ekf_t h, void* out);

/* SLAM_F32 or SLAM_F64, as given to slam_ekf_create. */
int slam_ekf_dtype(slam_ekf_t h, int* dtype);

/* A/B knob of the gating: SLAM_GATE_AUTO (the sweep below 16384 landmarks, the grid from there on), SLAM_GATE_SWEEP, SLAM_GATE_GRID.
 * The decisions are the same in every mode (tested). */
int slam_ekf_set_gate_mode(slam_ekf_t h, int mode);

/* out = {form of the last gating (SLAM_GATE_SWEEP / _GRID), grid cells per axis, landmarks in the grid, its tail, rebuilds, queries,
 * landmarks visited, landmarks evaluated} (counters since create). */
int slam_ekf_gate_info(slam_ekf_t h, int64_t out[8]);

/* enable = 1: every kernel launch is bracketed by HIP events on the handle's
 * stream; enable = a mask of (2 << SLAM_K_x): only those kernels (an event pair costs
 * ~10 us of stream time, so a benchmark brackets the dominant kernel only); 0: off.
 * timing_read synchronises, folds the pending events into per-kernel
 * totals and returns total milliseconds and launch count for kernel id `kid`. */
int slam_ekf_timing(slam_ekf_t h, int enable);

int slam_ekf_timing_read(slam_ekf_t h, int kid, double* total_ms, int64_t* launches);

/* The fastest bracketed launch of kernel `kid` since the last reset, in milliseconds (0: none).  Synchronises. */
int slam_ekf_timing_min(slam_ekf_t h, int kid, double* min_ms);

/* out = {bracketed launches, their mean, sample standard deviation and minimum in milliseconds} since the last reset.  Synchronises. */
int slam_ekf_timing_stats(slam_ekf_t h, int kid, double out[4]);

int slam_ekf_timing_reset(slam_ekf_t h);

/* Diagnostics: when enabled the factorisation kernel records 100 MHz wall-clock stamps at its
 * phase boundaries; out16 (may be NULL) receives the stamps of the last update: [0..7] the workgroup
 * that factors S, [8..15] the first of the workgroups that form W1 in the same launch (zero when
 * the update took the two-launch form). */
int slam_ekf_debug_stamps(slam_ekf_t h, int enable, uint64_t* out16);

/* Measurement hook (bench.py: roofline.copy_floor_ms): the bare memory side of the covariance down-date (src/ekf.jl:75) on
 * THIS handle's matrix -- every stored tile the down-date touches read once and written back unchanged (bit-exact), in
 * the down-date's own band-major order, no panels, no matrix-core work; `reps` individually timed passes of each of two launch
 * forms.  out = {milliseconds of the FASTEST pass, its form's index (0: one workgroup per tile, 1: persistent grid)}.  The
 * down-date's launch time over this figure compares across the boxes of a pool whose memory systems differ by a few
 * per cent.  Synchronises; the state is unchanged. */
int slam_ekf_copy_floor(slam_ekf_t h, int reps, double out[2]);

/* ---- map management: no counterpart in the reference ----------------------------------------------------------------------
 * The reference's map only grows (every observation outside gate2 becomes a landmark, src/data-association.jl).  For a
 * Gaussian, marginalising a landmark out is deleting its two rows / columns of P and its two entries of x: no arithmetic. */

/* Remove landmarks ids[0..cnt) (1-based, as idf; any order) from the map: x <- x[keep], P <- P[keep, keep], bit for bit;
 * the remaining landmarks keep their order and are renumbered 1..N-cnt.  new_index (may be NULL; N_old entries):
 * new_index[j-1] = the new id of old landmark j, 0 if it was removed.  cnt == 0: nothing happens.
 * In place on the device through a bounded staging buffer (<= 256 MiB); nothing below the first removed landmark moves.
 * SLAM_E_BADARG (state unchanged): null handle, cnt < 0, cnt > 0 with ids == NULL, an id outside 1..N, a duplicate id.
 * Ordered on the handle's stream behind everything enqueued before it (async updates included); synchronises. */
int slam_ekf_remove_landmarks(slam_ekf_t h, const int32_t* ids, int cnt, int32_t* new_index);

/* Duplicate landmarks.  Gated nearest-neighbour association enters a landmark a second time when the pose has drifted past
 * gate2 (the end of a long loop); from then on the map holds two landmarks for one feature.  For a < b (1-based), with
 * f(j) = 3 + 2 (j - 1):  delta = x[f(b) : f(b) + 2] - x[f(a) : f(a) + 2],  D = P_aa + P_bb - P_ab - P_ab' (the covariance of the
 * difference; evaluated in double from the stored values and symmetrised),  d2 = delta' inv(D) delta.  The pair is a duplicate
 * when D is positive definite as computed (D00 > 0 and det > 0) and d2 < gate.
 * *count = the number of duplicate pairs of the whole map; pairs receives the first min(count, cap) of them as (a, b), a < b,
 * in ascending lexicographic order (the same from call to call); pairs may be NULL when cap == 0.
 * A pair is first rejected from the means and the packed diagonal blocks alone (|delta|^2 >= 2 gate (tr P_aa + tr P_bb), which no
 * duplicate satisfies while the pair's joint covariance is positive semi-definite as stored); only the others read P_ab.
 * SLAM_E_BADARG: null handle, null count, cap < 0, cap > 0 with pairs == NULL, gate not finite or <= 0.
 * Ordered on the handle's stream behind everything enqueued before it; synchronises; the state is not changed. */
int slam_ekf_find_duplicates(slam_ekf_t h, double gate, int32_t* pairs, int cap, int* count);

/* Merge landmarks: pair p = (pairs[2p], pairs[2p + 1]) = (a_p, b_p) says "a_p and b_p are one point", the linear measurement
 * m_a - m_b = 0 with noise Rc (symmetric positive semi-definite 2 x 2, column-major as R; NULL = zero, the exact constraint).
 * All pairs of a call are ONE update in the reference's Cholesky form (src/ekf.jl:67-75): one pass over P however many pairs.
 * Then every b_p (the landmark named SECOND, whichever id is larger) is removed exactly as slam_ekf_remove_landmarks removes
 * it; the survivors keep their order.  new_index (may be NULL; N_old entries): as for removal for every survivor, and for a
 * removed b_p the NEW id of a_p.  cnt == 0: nothing happens.
 * SLAM_E_BADARG (state unchanged, decided before anything is enqueued): null handle, cnt < 0, cnt > SLAM_MERGE_MAX, cnt > 0 with
 * pairs == NULL, an id outside 1..N, a == b, a landmark in more than one pair of the call (merge a chain by calling again), Rc not
 * symmetric or with a negative diagonal.  SLAM_E_NOTPD: S is not positive definite (two landmarks already perfectly
 * correlated, with Rc = 0): state unchanged, nothing removed.
 * Ordered on the handle's stream behind everything enqueued before it (async updates included, whose deferred status stays
 * pending for slam_ekf_sync); synchronises. */
#define SLAM_MERGE_MAX 8      /* pairs per call: k = 16, one 16-column chunk of the down-date */
int slam_ekf_merge_landmarks(slam_ekf_t h, const int32_t* pairs, int cnt, const double Rc[4], int32_t* new_index);

/* The filter's HIP stream (interop: event timing around its kernels). */
int slam_pf_stream(slam_pf_t h, void** stream);

/* Collective: a barrier among the attached ranks through their inboxes; SLAM_OK when every peer's word arrived within
 * timeout_ms.  The caller's check, right after attaching, that the GPUs see each other's writes. */
int slam_pf_peer_selftest(slam_pf_t h, int timeout_ms);

/* out = {ranks, 1 if peers are attached, SLAM_PF_HALTED returns so far, resamplings so far}. */
int slam_pf_comm_info(slam_pf_t h, int64_t out[4]);

/* Diagnostics: 100 MHz wall-clock stamps of the last auto step: kernel start, every workgroup's statistics collected,
 * statistics folded, decision taken, bookkeeping done, published; [6] the collecting workgroup finished its own share,
 * [7] = [0] + 100 x the number of polls it needed.  Waits for the queue. */
int slam_pf_debug_stamps(slam_pf_t h, uint64_t out[8]);

/* ---- state read-outs ------------------------------------------------------------------------------------------------------
 * The FastSLAM map without downloading the particles: one pass over the landmark records WHERE THEY ARE (through the lazy
 * resampling's ancestor tables).  All three calls leave the auto mode as slam_pf_download does, honour a pending
 * normalisation shift and synchronise.  A filter that lives wholly on this shard is not changed in any way (no record moves,
 * its log-weights stay as stored); on a filter with peers attached the calls are COLLECTIVE: the remote records come home
 * first, as for slam_pf_download.  Results are the same bit for bit from call to call (fixed-order fp64 sums, no atomics).
 *
 * A particle contributes to landmark l only where its record is in use: Pxx > 0 (neither the Pxx = -1 mark of
 * slam_pf_clear_landmarks nor the all-zero record of a landmark never seen).  One exception: slam_pf_init_landmarks with
 * var = 0 writes used records with Pxx == 0; a record with Pxx == 0 counts when its landmark has been initialised or
 * observed by a known-correspondence call (the library's `seen` state), which no empty slot and no unseen landmark is.  w = exp(log-weight - pending shift), the weights
 * slam_pf_get_weights returns. */

/* The LOCAL sums, out[(1 + cnt) * 10] doubles; ids 1-based as in slam_pf_update_known, NULL = 1..nl (cnt ignored):
 *   row 0 (pose):      W, sum w x, sum w y, sum w x^2, sum w x y, sum w y^2, sum w sin(phi), sum w cos(phi), 0, n_local
 *   row 1 + i (ids[i]): W_l, sum w mx, sum w my, sum w mx^2, sum w mx my, sum w my^2, sum w Pxx, sum w Pxy, sum w Pyy, count_l
 * (W_l, count_l: weight mass and number of the contributing particles).  A sharded filter adds them over its ranks. */
int slam_pf_map_sums(slam_pf_t h, const int32_t* ids, int cnt, double* out);

/* The whole filter on this shard: out[cnt * 8] = {mass W_l / W, mean x, mean y, Cxx, Cxy, Cyy, count_l, 0} per landmark with
 * C = sum w P / W_l + (sum w m m' / W_l - mean mean'): the moment-matched Gaussian of the particles' mixture.  Mass 0: the
 * rest 0. */
int slam_pf_get_map(slam_pf_t h, const int32_t* ids, int cnt, double* out);

/* Local particle `idx` (-1: the one with the largest log-weight, the lowest index on a tie): its global id, log-weight, pose
 * and, if lm != NULL, its nl x 5 landmark records {x, y, Pxx, Pxy, Pyy} (row-major, double).  gid, logw, pose may be NULL. */
int slam_pf_get_particle(slam_pf_t h, int64_t idx, int64_t* gid, double* logw, double pose[3], double* lm);

/* ---- FastSLAM, unknown correspondences ---------------------------------------------------------------------------------------
 * predict + per-particle association + updates / new landmarks + local weight statistics as ONE sweep over the particles:
 * slam_pf_predict, slam_pf_update_unknown and slam_pf_weight_stats in one kernel, for m <= 64 (range, bearing) pairs.
 * Every observation is associated against the map as it is after the predict and before any of this call's updates; the
 * updates then run in observation order (a second observation of a slot sees the first one's update; a new landmark goes to the
 * particle's lowest unused slot, none left: dropped).  m <= 16: particles, decisions and statistics are those of the three
 * calls bit for bit (the same RNG step is consumed, a pending normalisation shift is honoured the same way).  m == 0: predict
 * and statistics only.  d_assoc (device, [m][n] int32, may be NULL): slot >= 0 matched, -1 new, -2 dropped.
 * out = {max logw, sum, sum2} as slam_pf_weight_stats.  SLAM_E_BADARG (state and RNG step unchanged): m < 0, m > 64, z == NULL
 * with m > 0.  Leaves the auto mode, materialises lazily resampled maps, is collective while peers are attached (all as
 * slam_pf_update_unknown); synchronises. */
int slam_pf_step_unknown(slam_pf_t h, double V, double G, double wheelbase, const double Q[4], double dt,
                         const double* z, int m, const double R[4], double gate1, double gate2,
                         int32_t* d_assoc, double out[3]);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_DIAG_H */
