/* slamhip_jc.h -- joint-compatibility data association for the EKF (joint compatibility branch and bound, Neira & Tardos 2001), the
 * entry points of the COMPANION library libslamhip_jc.so.  No counterpart in the reference, whose association is the
 * nearest neighbour of src/data-association.jl:1-63 (slam_ekf_associate, unchanged).
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_jc.so is built from csrc/ekf_jc.hip by the same Makefile, links against libslamhip.so (it works on that
 * library's handles) and is found beside it.  Same conventions: extern "C", int status codes, slam_last_error() of libslamhip.so
 * carries the message.
 *
 * THE RULE (tests/jc_ref.py runs it literally; the count of evaluated tests agrees with it).
 * 1. Candidates.  nis_ij is the normalised innovation squared of observation i against landmark j, as compute_association
 *    forms it (the double arithmetic of the gating sweep).  cand(i) is every landmark with nis_ij < gate1, sorted ascending by
 *    (nis, j); if there are more than SLAM_JC_MAXCAND the first SLAM_JC_MAXCAND are kept and `truncated` is set.  A NaN nis is
 *    never a candidate and never lowers a minimum.  min_i is the smallest nis_ij over all landmarks, +inf for an empty map.
 *    rem(i) is the number of observations i' > i with a non-empty cand.
 * 2. Search.  Depth first over i = 0 .. nz-1.  H is the current hypothesis and k its number of pairings.  Best starts empty
 *    with k = 0.
 *      - At i == nz: replace Best only if k > Best.k.  Among equal counts the first one found stands.
 *      - Otherwise, for each j in cand(i) in order, skipping any j already used in H:
 *          - if the number of tests evaluated so far equals max_nodes, set `exhausted` and stop the whole search;
 *          - count one test and form d2(H + (i, j));
 *          - the pairing is compatible iff every pivot is finite and positive and d2 < chi2[k] (strict); if so, descend with it.
 *      - After the candidates, descend with i unpaired iff k + rem(i) > Best.k.
 * 3. Decisions.  Paired observations of Best get their landmark.  An unpaired observation gets -1 iff min_i > gate2, else 0.
 *
 * The joint innovation is stacked in hypothesis order: v_(i,j) = z_i - zp_j with the bearing wrapped by mpi_to_pi.  The block of
 * the joint covariance S_H = H_H P H_H' + blockdiag(R) for landmarks j, j' is
 *     Hv_j Pvv Hv_j'' + Hv_j P[v,j'] Hf_j'' + Hf_j P[j,v] Hv_j'' + Hf_j P[j,j'] Hf_j'',   plus R on the diagonal blocks,
 * Hv / Hf the Jacobian blocks of predict_observation.  d2 = v' inv(S_H) v, from the Cholesky factor of S_H grown one pairing
 * (two rows) at a time; the pivots are that factor's squared diagonal.
 *
 * Common rules.  Both calls read the state and write nothing of it: x, P, the packed diagonal blocks and the grid stay unchanged
 * bit for bit.  They run on the handle's stream behind whatever is enqueued there and synchronise it (they produce host output).
 * All arithmetic is in double from the stored values of the handle's dtype.
 *
 * SLAM_JC_NODE_CAP.  The search is one dependent chain in one wave.  Measured on an MI355X (profiles/ekf_jc_bench.txt): a test at depth
 * 64 (a forward substitution through 126 rows) takes 20.2 us, at depth 32 10.5 us, at depth 8 3.7 us.  The cap keeps a call that
 * spends every node at depth 64 under one second: 40000 x 20.2 us = 0.81 s. */
#ifndef SLAMHIP_JC_H
#define SLAMHIP_JC_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_JC_MAXOBS   64
#define SLAM_JC_MAXCAND   8
#define SLAM_JC_NODE_CAP  40000

typedef struct slam_ekf_jc* slam_ekf_jc_t;

/* The search workspace of handle h (about 8.5 MB of device memory, plus 12 bytes per landmark and observation slot once a map is
 * searched).  h is borrowed: it must outlive the workspace, and the workspace is used from the thread that uses h.
 * SLAM_E_BADARG for a null argument, SLAM_E_NOMEM / SLAM_E_HIP from the runtime. */
int slam_ekf_jc_create(slam_ekf_jc_t* jc, slam_ekf_t h);
int slam_ekf_jc_destroy(slam_ekf_jc_t jc);

/* The rule above for the nz observations z (range, bearing pairs) under the noise R (column-major 2 x 2).
 *   chi2[k-1]  the threshold for a hypothesis of k pairings: the chi-square quantile with 2k degrees of freedom; nz values
 *   max_nodes  the most joint tests the search may evaluate, 1 .. SLAM_JC_NODE_CAP
 *   assoc[nz]  as in slam_ekf_associate: j >= 1 matched landmark, 0 dropped, -1 new feature
 *   info[8]    {pairings of the result, its d2, joint tests evaluated, exhausted (0/1), truncated (0/1), distinct candidate
 *               landmarks, deepest hypothesis tested (pairings), 0}
 * SLAM_E_BADARG, with nothing enqueued: a null argument (z, chi2 and assoc may be null when nz == 0), nz outside 0 .. SLAM_JC_MAXOBS, a
 * non-finite R, gate or chi2 entry, max_nodes < 1 or > SLAM_JC_NODE_CAP. */
int slam_ekf_associate_joint(slam_ekf_jc_t jc, const double* z, int nz, const double R[4], double gate1, double gate2,
                             const double* chi2, int64_t max_nodes, int32_t* assoc, double info[8]);

/* d2 = v' inv(S_H) v of the caller's hypothesis: observation i (z[2i], z[2i+1]) is paired with the 1-based landmark idf[i],
 * 1 <= m <= SLAM_JC_MAXOBS, the ids distinct and in 1 .. N (anything else: SLAM_E_BADARG, nothing enqueued).
 * SLAM_E_NOTPD when a pivot of S_H is not positive (d2 is then not written). */
int slam_ekf_joint_nis(slam_ekf_jc_t jc, const double* z, const int32_t* idf, int m, const double R[4], double* d2);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_JC_H */
