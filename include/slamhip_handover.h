/* slamhip_handover.h -- a state handed from one filter to the other on the device: the particles of a FastSLAM filter collapsed
 * into the joint Gaussian an EKF handle holds (slam_pf_to_ekf), and a particle filter seeded from an EKF state
 * (slam_ekf_to_pf).  The entry points of the COMPANION library libslamhip_handover.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_handover.so is built from csrc/handover.hip by the same Makefile, links against libslamhip.so (it works
 * on that library's handles and calls its internal helpers: both come from one tree and one make) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message.
 *
 * Both calls need equal dtypes, equal devices, and a particle filter that lives wholly on one shard (n_local == n_global)
 * without peers: SLAM_E_BADARG otherwise.  SLAM_E_CAPACITY where the result does not fit dst.  On every error decided before
 * dst is written both states are unchanged bit for bit (the RNG step and the pending normalisation shift included; a filter in
 * auto mode is left as slam_pf_download leaves it).  Ordering between the two handles as slam_ekf_join / slam_ekf_copy: the
 * work is enqueued on dst's stream behind an event recorded on src's stream, and an event recorded on dst's stream after the
 * last read of src is made a dependency of src's stream.  Both calls synchronise.
 *
 * ============================ PARTICLES -> EKF (tests/handover_ref.py: pf_to_ekf runs it literally) ============================
 * w_i = exp((T)(logw_i - pending shift)) in fp64 -- the weights slam_pf_get_weights returns --, W = sum w_i, what_i = w_i / W,
 * Neff = W^2 / sum w_i^2.  A particle's vector is z_i = (x, y, phi, m_1x, m_1y, ..., m_N'x, m_N'y), landmark k of dst being
 * slot ids[k - 1] of src.
 *   mean        mu_x = sum what x, mu_y = sum what y, mu_phi = atan2(sum what sin phi, sum what cos phi) (circular, the
 *               convention of slam_pf_mean_pose_sums), landmark means sum what m.  The sums are the fixed-order fp64 sums of
 *               slam_pf_map_sums: this call takes its first pass from that read-out, so means, the within-particle term and
 *               the counts below are the numbers slam_pf_get_map is formed from.
 *   deviations  d_i = z_i - mu in fp64, the heading component through the single conditional mpi_to_pi.
 *   covariance  P = sum what_i d_i d_i' + blockdiag(0_3, sum what_i P_i,1, ..., sum what_i P_i,N')      (law of total covariance)
 *               P_i,k the particle's 2 x 2 landmark block.  Symmetric; inside a diagonal tile one owner writes an entry and
 *               its mirror.
 *   identity    every chosen landmark must be in use in EVERY particle (the "in use" test of slam_pf_map_sums: Pxx > 0, or
 *               Pxx == 0 for a landmark in the `seen` state), i.e. count_l == n.  A short count -- a filter run with unknown
 *               correspondences, a landmark never seen -- is SLAM_E_BADARG with the landmark named; W == 0 or not finite too.
 * src AFTERWARDS: its records may have been materialised (as slam_pf_update_unknown does); what slam_pf_download returns is
 * unchanged bit for bit, the log-weights stay as stored, the pending shift stays pending.
 * dst AFTERWARDS, exactly as slam_ekf_copy leaves it: N', x[0 : n'), P; every tile row below Tw = min(T_dst, ceil(max(n_old,
 * n') / E)) is written completely, +0.0 outside n'; the packed 2 x 2 side array is rebuilt; the panel workspace is zeroed when
 * N shrinks; the variance bound and the grid are marked stale.
 *
 * THE SUMMATION STRUCTURE (what the error bound of tests/handover_ref.py and DESIGN 5.10 rests on).  T = the handle's dtype,
 * u = its unit roundoff (2^-24 / 2^-53), E = 128 (fp32) / 64 (fp64) the EKF's tile edge.
 *   1. sw_k = (T) sqrt(what_k), the square root in fp64.                                     one rounding to T
 *   2. Y[k][a] = (T)(z_ka - mu_a) * sw_k: the difference (and the wrap) in fp64, rounded to T once, the product in T.
 *                                                                                            two roundings to T
 *   3. The particle axis is cut into slabs of SLAM_HANDOVER_SLAB_F32 = 8192 (fp32) / SLAM_HANDOVER_SLAB_F64 = 4096 (fp64)
 *      particles.  One workgroup per (tile, slab) forms the E x E partial sum_k Y[k][a] Y[k][b] over its slab on the matrix
 *      cores: v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, each entry ONE k-ordered chain of fused multiply-adds in T
 *      (one rounding per term, no wider accumulator), at most SLAB terms long.  The partial is stored in T.
 *   4. One thread per entry adds the slabs' partials in slab order in fp64, adds the within-particle term (fp64, from the sums of
 *      pass 1) on the 2 x 2 diagonal blocks, rounds to T once and stores at p_off (an entry of a diagonal tile with r >= c
 *      also at its mirror).
 * No floating-point atomics: the result is the same bit for bit from call to call.  Per entry
 *   |P_ab - exact| <= gamma (sum_k what_k |d_ka| |d_kb|) + u |P_ab| + (fp64 terms),    gamma = (SLAB + 8) u
 * (6 u for the inputs of step 1 and 2 in both factors, SLAB u for the chain, 2 u slack); tests/handover_ref.py has the derivation
 * with the fp64 terms written out.
 * The partials, sw, the means and the work list live in src's grow-only read-out scratch (the one slam_pf_map_sums uses; an EKF
 * handle has no scratch of that size): nothing is allocated per call once it is warm.  All offsets are 64-bit.
 *
 * ============================ EKF -> PARTICLES (tests/handover_ref.py: ekf_to_pf runs it literally) ============================
 * A first, tiny launch works in fp64 from the handle's values: L_v = chol(P_vv) (3 x 3 lower), and for landmark j of dst (slot
 * ids[j - 1] of src, f = 3 + 2 (ids[j - 1] - 1)):  B_j = P[f : f + 2, 0 : 3] P_vv^-1 by two triangular solves,
 * C_j = P_jj - B_j P[f : f + 2, 0 : 3]' with the LOWER entry P[f + 1, f] as the off-diagonal.  A pivot <= 0, C_j,xx <= 0 or
 * det C_j <= 0 is SLAM_E_NOTPD: read back before anything of dst is written, dst unchanged.  A vehicle that is known exactly has
 * P_vv = 0 and is refused that way: such a caller uses slam_pf_set_pose plus slam_pf_init_landmarks.
 * Particle with global id g: three standard normals from Philox4x32-10, counter (g lo, g hi, step, STREAM_HANDOVER = 3), key =
 * the seed; (xi_0, xi_1) = Box-Muller on words 0 and 1 exactly as the filter's normals2, xi_2 = the first Box-Muller output of
 * words 2 and 3.  With every table value rounded to T and every operation in T, left to right, no contraction:
 *   delta_0 = L00 xi_0,  delta_1 = L10 xi_0 + L11 xi_1,  delta_2 = (L20 xi_0 + L21 xi_1) + L22 xi_2
 *   pose = x_v + delta, the heading through mpi_to_pi
 *   record j = (m_jx + ((B00 delta_0 + B01 delta_1) + B02 delta_2), m_jy + (...), C_xx, C_xy, C_yy)
 *   log-weight = -log n as slam_pf_set_pose stores it.
 * dst AFTERWARDS: landmarks 1 .. cnt in the `seen` state, every other slot as slam_pf_create leaves it (the all-zero record, not
 * seen); lazy ancestor tables released, the pending shift dropped, auto mode left; the resample count unchanged; the RNG step
 * advanced by one.  One pass writes the records [lm][5][n], 16-byte stores where n is a multiple of 4. */
#ifndef SLAMHIP_HANDOVER_H
#define SLAMHIP_HANDOVER_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_HANDOVER_SLAB_F32 8192
#define SLAM_HANDOVER_SLAB_F64 4096

/* dst <- the moment-matched joint Gaussian of the particles of src over the pose and the landmarks ids[0..cnt)
 * (1-based, distinct, any order; ids == NULL: every landmark in the library's `seen` state, ascending, cnt ignored).
 * info (may be NULL) = {W, Neff, n, N'}.  Synchronises. */
int slam_pf_to_ekf(slam_ekf_t dst, slam_pf_t src, const int32_t* ids, int cnt, double info[4]);

/* dst <- n particles drawn from the EKF state src: the pose from the vehicle marginal, every landmark the conditional given that pose.
 * ids as above over src's landmarks (NULL: 1..N).  Consumes one RNG step of dst.  Synchronises. */
int slam_ekf_to_pf(slam_pf_t dst, slam_ekf_t src, const int32_t* ids, int cnt);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_HANDOVER_H */
