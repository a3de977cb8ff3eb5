/* slamhip_pfcopy.h -- a FastSLAM particle set moved on the device: uploaded, copied, selected and resized between handles, and the
 * pose histogram that KLD-sampling sizes a filter by.  The entry points of the COMPANION library libslamhip_pfcopy.so, the
 * FastSLAM twin of slamhip_copy.h.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_pfcopy.so is built from csrc/pf_copy.hip by the same Makefile, links against libslamhip.so (it works on
 * that library's handles and calls its internal helpers: both come from one tree and one make) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message.
 *
 * THE CALLS BETWEEN TWO HANDLES (slam_pf_select, slam_pf_copy, slam_pf_resize) need equal dtypes and equal devices, dst != src,
 * and two filters that each live wholly on one shard without peers (n_local == n_global, first_id == 0): SLAM_E_BADARG
 * otherwise.  SLAM_E_CAPACITY where the result does not fit dst.  On every error decided before dst is written both states
 * are unchanged bit for bit (the RNG state and a pending normalisation shift included; a filter in auto mode is left as
 * slam_pf_download leaves it: the queue has been waited for and the bookkeeping is back on the host).  Ordering between the
 * two handles as slam_ekf_copy / slam_pf_to_ekf: the work is enqueued on dst's stream behind an event recorded on src's
 * stream, and an event recorded on dst's stream after the last read of src is made a dependency of src's stream.  All three
 * synchronise dst's stream before they return.
 *
 * WHERE A RECORD LIES.  Landmark l's record of particle p of a filter lies in buffer lbuf[l] at slot tab[ltab[l]][p] (slot p
 * without a table): lazy resampling.  The three calls read every record of src WHERE IT LIES -- src is only read, it is not
 * even materialised, its log-weights stay as stored and its shift stays pending -- and write it plain into dst's buffer
 * `cur`.  dst AFTERWARDS has plain maps: every ancestor table released, lbuf = cur, nothing lazily pending, exactly the
 * bookkeeping of slam_pf_clear_landmarks and of slam_ekf_to_pf; no pending shift.
 *
 * ============================ SELECT AND COPY (tests/pfcopy_ref.py: select runs it literally) ============================
 * dst.n == src.n.  Landmark k (1-based) of dst is slot ids[k - 1] of src, k = 1 .. cnt; ids 1-based, distinct, any order, each in
 * 1 .. src.max_landmarks; ids == NULL means 1 .. src.max_landmarks (cnt ignored).  cnt > dst.max_landmarks: SLAM_E_CAPACITY.
 *   records     dst(k, row, p) = src(ids[k - 1], row, p), all five rows, every value bit for bit (negative zeros, denormals and
 *               NaN payloads included: the values move as integers), and seen_dst[k] = seen_src[ids[k - 1]].
 *   fill        slots k > cnt:  fill = 0  the all-zero record, not seen, as slam_pf_create leaves it;
 *                               fill = 1  the unused record (0, 0, -1, 0, 0), not seen, as slam_pf_clear_landmarks leaves it:
 *                                         what a filter with unknown correspondences needs.  Anything else: SLAM_E_BADARG.
 *   poses       dst.pose(row, p) = src.pose(row, p) bit for bit.
 *   log-weights dst.logw[p] = (T)(src.logw[p] - (T) pending shift) when src has a shift pending, the stored bits otherwise: the
 *               values slam_pf_download(src) returns.  dst has no pending shift; src's stays pending.
 *   RNG         dst takes over src's seed, RNG step and resample count: a clone that is driven like the original stays equal
 *               to it bit for bit.
 * slam_pf_copy(dst, src, fill) is slam_pf_select with ids = 1 .. src.max_landmarks; it needs dst.max_landmarks >=
 * src.max_landmarks (SLAM_E_CAPACITY otherwise; a smaller destination goes through slam_pf_select).
 *
 * ============================ RESIZE (tests/pfcopy_ref.py: resize and ExactInto) ============================
 * m = dst.n, n = src.n, any two counts (m == n gives a resampled clone and leaves src alone).  dst.max_landmarks >=
 * src.max_landmarks (SLAM_E_CAPACITY otherwise); all of src's landmarks are taken, `seen` follows, the remaining slots follow
 * `fill`.  0 <= u0 < 1.
 *   weights     w_i = exp((double)(T)(logw_i - (T) pend) - gmax) in fp64, pend = src's pending shift or 0: exactly the weights
 *               slam_pf_resample_local forms.
 *   cdf         block_scan1024 inside blocks of 1024 particles (csrc/pf_device.h: Hillis-Steele over the 64 lanes of a wave,
 *               the wave totals added in wave order), the blocks' offsets added serially in block order from 0.0; the value
 *               compared is cdf_j = scan_j + offset[j / 1024], total = the last offset.  The scan of slam_pf_resample_local.
 *   target      slot q of dst:  t_q = fl(fl(fl(q + u0) / m) * total)            (m, not n)
 *   ancestor    anc[q] = the first j in [0, n) with cdf_j >= t_q (binary search; j = n - 1 when none).
 *   particles   dst particle q = src particle anc[q]: the pose and every landmark record bit for bit, read in place through
 *               src's lazy tables.
 *   log-weights (T)(-log m), as slam_pf_set_pose stores them.
 *   RNG         seed and RNG step are taken over; the resample count becomes src's plus one.
 * total not finite or <= 0 is SLAM_E_BADARG, read back before anything of dst is written.  anc (host, m int32, may be NULL)
 * receives the table.  No floating-point atomics: the result is the same bit for bit from call to call.  The table is
 * non-decreasing wherever the stored cdf is (see block_scan1024 on its one-ulp descents).
 *
 * THE GATHER (csrc/pf_copy.hip: pc_gather_kernel, one kernel family for the three calls).  dst(k, q) = src(slot_k, anc_q), anc the
 * identity for select and copy.  A per-landmark work list {source slot or fill code, table + 1 | buffer << 8} is uploaded into
 * dst's grow-only read-out scratch and read wave-uniformly.  Grid (slabs of 1024 particles) x (groups of 16 dst landmarks); a
 * thread owns four dst particles, loads their ancestors once and a table's entries once per run of landmarks behind that
 * table; group 0 also moves the poses and the log-weights.  m a multiple of 4: the four particles are consecutive, 16-byte
 * stores, and 16-byte loads where the ancestors are the identity and the landmark has no table (4-byte / 8-byte gathers
 * otherwise); any other m: the thread's particles are 256 apart, scalar stores.  The stores are non-temporal.  All offsets
 * are 64-bit; both handles are addressed through their own chunk tables (the two chunk shifts may differ).
 *
 * ============================ UPLOAD, META, RNG ============================
 * slam_pf_upload is the inverse of slam_pf_download: host buffers in the handle's dtype, pose [3][n], logw [n], lm [nl][5][n],
 * seen [nl] bytes (0 / not 0).  pose and logw may each be NULL (that part stays); lm and seen are given together or both NULL.
 * The landmarks go chunk by chunk into buffer cur; with lm given the maps are plain afterwards (tables released, lbuf = cur,
 * nothing lazily pending: the bookkeeping of slam_pf_clear_landmarks).  With logw given a pending normalisation shift is
 * dropped.  Auto mode is left.  The values are stored as given: no validation beyond the arguments.  Works on a shard
 * (n_local < n_global) as long as no peers are attached (SLAM_E_BADARG with peers).  Synchronises.
 *
 * ============================ POSE BINS (tests/pfcopy_ref.py: pose_bins) ============================
 * The number k of distinct occupied cells of the pose histogram (KLD-sampling, Fox 2003).  In fp64 from the stored values:
 *   ix = floor(x / cell_xy), iy = floor(y / cell_xy), ip = floor((phi + pi) / cell_phi) clamped to [0, ceil(2 pi / cell_phi) - 1]
 * with pi = 3.14159265358979323846.  |ix| or |iy| >= 2^20, a pose that is not finite, a cell that is not positive (or not
 * finite), or more than 2^21 heading cells: SLAM_E_BADARG.  One open-addressing set of 64-bit keys ((ix + 2^20) << 42 |
 * (iy + 2^20) << 21 | ip) of 2 next_pow2(n) slots in the filter's grow-only read-out scratch, linear probing, an ordinary
 * compare-and-swap insert; whoever inserts a new key raises the count, so the count does not depend on the order.  The filter
 * is only read (auto mode is left).  Synchronises. */
#ifndef SLAMHIP_PFCOPY_H
#define SLAMHIP_PFCOPY_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = {n_local, n_global, first_id, max_landmarks, dtype, RNG step, resample count, seed as its bit pattern}; seen (may be
 * NULL) receives the per-landmark `seen` flags, max_landmarks bytes.  Waits for the queue of an auto-mode filter and leaves it
 * as slam_pf_download does. */
int slam_pf_get_meta(slam_pf_t h, int64_t out[8], uint8_t* seen);

/* The Philox key and the step counter.  (The resample count has its setter in slamhip.h: slam_pf_set_resample_count.) */
int slam_pf_set_rng(slam_pf_t h, uint64_t seed, uint32_t step);

/* The inverse of slam_pf_download (see above).  Synchronises. */
int slam_pf_upload(slam_pf_t h, const void* pose, const void* logw, const void* lm, const uint8_t* seen);

/* dst <- src with landmark k of dst = slot ids[k - 1] of src (see above).  Synchronises. */
int slam_pf_select(slam_pf_t dst, slam_pf_t src, const int32_t* ids, int cnt, int fill);

/* dst <- src, every landmark in its place.  Synchronises. */
int slam_pf_copy(slam_pf_t dst, slam_pf_t src, int fill);

/* dst (m particles) <- src (n particles) by systematic resampling into m slots (see above).  anc: host, m int32, may be NULL.
 * Synchronises. */
int slam_pf_resize(slam_pf_t dst, slam_pf_t src, double gmax, double u0, int fill, int32_t* anc);

/* *bins = the number of distinct occupied cells of the pose histogram (see above).  Synchronises. */
int slam_pf_pose_bins(slam_pf_t h, double cell_xy, double cell_phi, int64_t* bins);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_PFCOPY_H */
