/* slamhip_proposal.h -- FastSLAM 2.0 with UNKNOWN correspondences (Montemerlo et al. 2003): every particle associates this step's
 * observations with its own landmarks under the prior proposal, draws its pose from the proposal that knows the matched
 * observations, and updates its map from the sampled pose.  The entry points of the EXTENSION library libslamhip_proposal.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare, and none of its kernels changes.  libslamhip_proposal.so is built from csrc/pf_proposal.hip by the same Makefile, links
 * against libslamhip.so (it works on that library's particle handles) and is found beside it.  Same conventions: extern "C", int
 * status codes, slam_last_error() of libslamhip.so carries the message.
 *
 * LIMITS: 0 <= m <= SLAM_PF_PROPOSAL_MAXOBS (16) observations per call; the whole filter on one shard (n_local == n_global, no
 * peers attached); the calls leave the auto mode (slam_pf_step_auto) first; the step call synchronises.
 *
 * THE RULE (tests/proposal_unknown_ref.py runs it literally in fp64).  For every particle, with its stored pose (x, y, phi), its
 * log-weight minus the pending normalisation shift, and its map as it is BEFORE this call:
 *
 *  1. Mean motion and GL, exactly as slam_pf_step_proposal forms them: Lq = chol((Q + Q') / 2) lower,
 *       s, c = sin, cos(G + phi);  xm = x + V dt c,  ym = y + V dt s,  pm = mpi_to_pi(phi + V dt sin(G) / wheelbase)
 *       GL = Gu Lq (3 x 2), Gu the Jacobian of the motion model in the control (src/ekf.jl:27-29).
 *
 *  2. Association at the mean pose, under the PRIOR proposal.  For every slot l in use (Pxx >= 0) and every observation i:
 *       dx = lx - xm, dy = ly - ym, d2 = dx dx + dy dy, d = sqrt(d2), zp1 = atan2(dy, dx) - pm
 *       Hf = [dx / d, dy / d; -dy / d2, dx / d2]                                 (src/common.jl:162)
 *       B  = Hv GL, Hv = [-h00 -h01 0; -h10 -h11 -1]:   b00 = -(h00 gl00 + h01 gl10), b01 = -(h00 gl01 + h01 gl11),
 *                                                       b10 = -(h10 gl00 + h11 gl10) - gl20, b11 = -(h10 gl01 + h11 gl11) - gl21
 *       S  = (Hf Pf Hf' + R) + B B', NOT symmetrised: the first bracket entry by entry as slam_pf_update_unknown forms it, then
 *            s00 += b00 b00 + b01 b01,  s01 += b00 b10 + b01 b11,  s10 += b10 b00 + b11 b01,  s11 += b10 b10 + b11 b11
 *            (B B' is the pose uncertainty before any observation: Sigma = I in control space)
 *       det = s00 s11 - s01 s10;  qa = s11 / det, qb = -(s01 + s10) / det, qc = s00 / det;  logdet = log(det)
 *       v0 = r_i - d, v1 = mpi_to_pi(b_i - zp1);  nis = qa v0 v0 + qb v0 v1 + qc v1 v1;  nd = nis + logdet
 *     Decision, as slam_pf_update_unknown: among the slots with nis < gate1 the smallest nd wins, the lowest slot wins a tie;
 *     otherwise -2 if any slot has nis <= gate2, else -1.  All observations are associated against the map before this call.
 *     (These quantities use exact sqrt / atan2 / log / divisions in fp32 too, as slam_pf_update_unknown does.)
 *
 *  3. Proposal.  The matched observations, in observation order, are assimilated as linear 2 x 2 measurements of the control noise
 *     w ~ N(0, I), exactly as slam_pf_step_proposal does for a landmark the particle holds (B, Sf symmetrised, S = B Sig B' + Sf,
 *     the Cholesky form, mu, Sig, the guard that keeps Sig positive semi-definite).  The landmark is the particle's own slot, read
 *     from the PRIOR map: two observations matched to one slot both read the prior record.  Each matched observation adds its
 *     predictive log-density to the log-weight.  Decisions -1 and -2 touch neither the proposal nor the weight.
 *
 *  4. Draw.  w = mu + chol(Sig) e with the two normals of the predict stream at the handle's step (the step counter then advances
 *     by one, as in every step call); the pose follows by the exact motion model under V + (Lq w)_0, G + (Lq w)_1.
 *
 *  5. Apply, in observation order, from the SAMPLED pose, the weight left alone: a matched observation runs the landmark update
 *     on its slot (a second observation of the slot sees the first one's update); a new one (-1) initialises the particle's lowest
 *     unused slot; if none is left the observation is dropped and reported as -2.
 *
 *  6. out[3] = {max log-weight, sum exp(logw - max), sum exp(2 (logw - max))}: what slam_pf_weight_stats would return right after
 *     the call, bit for bit.  d_assoc (device, [m][n] int32, may be NULL): slot >= 0 matched, -1 new, -2 dropped.
 *
 * With m == 0 the step is slam_pf_step_unknown with m == 0 bit for bit when Q is diagonal; on a map without landmarks it is
 * slam_pf_step_unknown bit for bit when Q is diagonal.
 *
 * slam_pf_associate_proposal runs steps 1 and 2 only.  Poses, weights, records, the RNG step and a pending normalisation are only
 * read (lazily resampled records are brought to their particles' slots first, which changes no value a read-out returns).
 * d_assoc as above, the decision of step 2 (the capacity of step 5 is not consulted); d_nis (device, [m][n] in the handle's
 * dtype, may be NULL): the nis of the winning slot, NaN where nothing matched.  Enqueued on the handle's stream.
 *
 * SLAM_E_BADARG, decided before anything is enqueued -- state and RNG step are unchanged: a null handle, Q or out; z or R null
 * with m > 0; m outside 0 .. 16; V, G, wheelbase, dt, a gate, an entry of Q, R or z not finite; Q not positive definite; a handle
 * that is not the whole filter (n_local != n_global, or peers attached).
 */
#ifndef SLAMHIP_PROPOSAL_H
#define SLAMHIP_PROPOSAL_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_PF_PROPOSAL_MAXOBS 16

int slam_pf_step_proposal_unknown(slam_pf_t h, double V, double G, double wheelbase, const double Q[4], double dt, const double* z,
                                  int m, const double R[4], double gate1, double gate2, int32_t* d_assoc, double out[3]);

int slam_pf_associate_proposal(slam_pf_t h, double V, double G, double wheelbase, const double Q[4], double dt, const double* z,
                               int m, const double R[4], double gate1, double gate2, int32_t* d_assoc, void* d_nis);

/* out = {SLAM_PF_PROPOSAL_MAXOBS, 0, 0, 0} */
int slam_pf_proposal_limits(int out[4]);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_PROPOSAL_H */
