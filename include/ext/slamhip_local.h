/* slamhip_local.h -- compressed local-area updates for the EKF (Guivant & Nebot, IEEE Trans. Robotics & Automation 17(3),
 * 2001): while the vehicle works among a few landmarks, every predict, update and add_features runs on a SMALL state, three small
 * accumulators are carried alongside, and the rest of the map is brought up to date in ONE pass when the area is closed.  Up to
 * rounding the result is what the full filter would have produced step by step: the scheme is exact, not an approximation.  The
 * entry points of the EXTENSION library libslamhip_local.so.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_local.so is built from csrc/ekf_local.hip by the same Makefile, links against libslamhip.so (it works on
 * that library's handles and reads their update workspace) and against libslamhip_copy.so (open IS slam_ekf_select), and is
 * found beside them.  Same conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message.
 * The header lives in include/ext/ and is found through the same -I as the others.
 *
 * THE RULE (tests/local_ref.py runs it literally).  The global state is (x, P), n = 3 + 2 N.  open(ids, cnt) chooses cnt
 * distinct global landmarks (1-based, any order).  A = the vehicle plus those landmarks, n0 = 3 + 2 cnt; B = everything else.
 * Local landmark j (1-based) is global ids[j - 1].  The object keeps a local EKF handle -- after open bit for bit what
 * slam_ekf_select(local, global, ids, cnt) gives -- and three accumulators in DOUBLE whatever the state's dtype:
 *     phi    n_a x n0   = I at open        (n_a = 3 + 2 (cnt + landmarks added locally) is the local state's size)
 *     psi    n0 x n0    = 0
 *     theta  n0         = 0
 * with the invariant  P_ab(now) = phi P_ab(at open).
 *   predict (v, g, wheelbase, Q, dt)   Gv = [1 0 -v dt sin(g + p); 0 1 v dt cos(g + p); 0 0 1] with p the local heading before the
 *                             step, the Jacobian slam_ekf_predict applies:  phi[0:3, :] <- Gv phi[0:3, :];  then slam_ekf_predict
 *                             on the local handle.  psi and theta are untouched.
 *   update (z, idf, m, R)     Cholesky form only.  idf are LOCAL ids in 1 .. n_a's landmarks.  H = the 2m x n_a Jacobian at the
 *                             local state BEFORE the update (5 non-zeros a row), E = H phi (k x n0, k = 2m).  Then slam_ekf_update
 *                             on the local handle, which leaves in its workspace C = inv(chol(S))' (upper), g = C C' v and W, the
 *                             panel its down-date used (W1 = P H' C rounded once to the state's dtype).  With Y = C' E:
 *                                 theta += E' g        psi += Y' Y        phi -= W Y
 *                             psi's term is formed as E' (C (C' E)), the same product; every sum in double, ascending index.
 *                             All three come from the workspace for EVERY k (the fused factor launch, the separate W1 launches
 *                             and the large-k path all leave C, g and W1 behind): nothing is recomputed from P_aa.
 *   augment (zn, nn, R)       for each new observation (r, b) at local heading p: Gxv = [1 0 -r sin(p + b); 0 1 r cos(p + b)],
 *                             phi gains the two rows Gxv phi[0:3, :]; then slam_ekf_augment on the local handle.
 *   close                     with A0 = P_ba(at open) (n_b x n0), in this order
 *                                 1. x_b  += A0 theta
 *                                 2. P_bb -= (A0 psi) A0'      the stored entries: the tiles on and below the diagonal; inside a
 *                                                              diagonal tile the entry with r >= c is formed and its mirror gets
 *                                                              the same value
 *                                 3. P_ab <- phi A0'           rows of landmarks added locally are appended as global N + 1 ...,
 *                                                              in the order they were added
 *                                 4. x_a, P_aa <- the local state, scattered to ids and to the appended rows, bit for bit
 *                                 5. N grows
 *                             Afterwards the packed diagonal blocks (slam_ekf_get_landmark_blocks) agree with the matrix, the
 *                             gating grid is marked for rebuild, the pre-gate's variance bound is invalidated, and *first_new is
 *                             the global id of the first appended landmark (N + 1 also when none was added).
 *   abort                     discards the area: the global state is bit for bit untouched (it was never written).
 *
 * THE CONTRACT.  While an area is open the GLOBAL handle must not be written: close checks that N is what it was at open and
 * returns SLAM_E_BADARG otherwise (anything else a caller wrote is not detected).  The LOCAL handle (slam_ekf_local_state) is
 * written only through this library; it may be read freely: slam_ekf_associate, slam_ekf_associate_joint, slam_ekf_nis,
 * slam_ekf_get_state and the other read-outs work on it unchanged.  Observations of landmarks in B cannot be used until close.
 * One area per object at a time; several objects over one global handle are the caller's business (their closes do not commute).
 *
 * NOT POSITIVE DEFINITE.  A local update whose S fails returns SLAM_E_NOTPD; the local state is bit for bit what it was (the
 * product's guarantee) and so are phi, psi and theta: the accumulator launch behind the update reads the same device status word
 * the down-date returns on.  SLAM_FORM_JOSEPH is SLAM_E_BADARG.
 *
 * SYNCHRONISATION.  predict, update and augment enqueue on the LOCAL handle's stream one accumulator launch before the product
 * call (E = H phi; the Gv / Gxv row operations) and, for update, one after it (Y and the three rank-k updates), and do not
 * synchronise beyond what the wrapped product call does (slam_ekf_update reads its status back unless the local handle is in
 * async mode).  open is enqueued like slam_ekf_select.  close orders the global stream behind the local one and the local one
 * behind close's last read, enqueues its chain on the GLOBAL handle's stream and SYNCHRONISES it.  get and info synchronise.
 *
 * THE LAUNCH CHAIN OF close.  Every dependency is a launch boundary: no workgroup waits for another, no ready words, no atomics.
 *     gather   A0[r, j] = P[r, a(j)] for EVERY global row r < n (symmetric view), column-major n_pad x K in the state's dtype T,
 *              K = n0 rounded up to 16, zero outside; the values are P's own, so nothing is rounded
 *     T = A0 psi     one entry = ONE chain of n0 fused multiply-adds in double, j ascending, rounded once to T.  The rows of T
 *              that belong to A are written as ZERO, so the trailing product below runs over one uniform tile grid and leaves
 *              the rows of A alone (their columns are rewritten by the scatter)
 *     x_b      x[r] = (T)(x[r] + sum_j A0[r, j] theta[j]), double, j ascending, r in B
 *     trail    P[r, c] -= sum_k T[r, k] A0[c, k] over the lower tile grid of the old state on the matrix cores:
 *              v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, operands in T, each entry ONE k-ordered chain of K fused
 *              multiply-adds in the accumulator of that dtype, then one subtraction in T.  Operands go from global memory
 *              straight into the MFMA, a wave owning a quadrant of the tile as 2 x 2 blocks (the trailing update of
 *              slam_ekf_factor_compute).
 *     A1 = A0 phi'   n x n_a, the same kernel as T: one double chain of n0 terms, rounded once to T
 *     scatter  rows of B take A1, rows of A take the local state; an entry of a diagonal tile and its mirror have one writer
 *     side     the packed 2 x 2 diagonal blocks are rebuilt from the matrix
 *
 * THE BOUND of close, per entry, against the EXACT result of the five steps above applied to close's own inputs (the global
 * state, the local state and phi, psi, theta as slam_ekf_local_get returns them).  u = the state's unit roundoff (2^-24 / 2^-53),
 * v = 2^-53, gamma(k, w) = k w / (1 - k w), |.| entrywise absolute values:
 *     x_b    |err_r|   <= u |x_r'| + gamma(n0 + 1, v) (|x_r| + sum_j |A0_rj| |theta_j|)
 *     P_bb   |err_rc|  <= u |P_rc'| + (gamma(K + 1, u) + u) sum_k |T_rk| |A0_ck| + (1 + u) gamma(n0, v) sum_k (|A0| |psi|)_rk |A0_ck|
 *                       u |P'|: the final subtraction; gamma(K + 1, u): the chain on the matrix cores, K terms in any order,
 *                       fused or not; u: T rounded once to the state's dtype (|T| here is T as computed, i.e. at most
 *                       (1 + u) |A0 psi| plus the last term's chain error); the last term: the double chain behind every T_rk
 *     P_ab   |err_ri|  <= u |P_ri'| + gamma(n0, v) sum_j |A0_rj| |phi_ij|
 *     x_a, P_aa        exact copies.
 * (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1, for the chains.)  What the INPUTS carry -- the local
 * filter's own rounding, which is the product's: slam_ekf_predict / _update / _augment on a small handle -- is not part of this
 * bound; tests/test_gpu_ekf_local.py measures the whole sequence against the fp64 oracle beside the product's full path.
 *
 * STATUS CODES, decided on the host before anything is enqueued, everything unchanged:
 *   SLAM_E_BADARG    a null argument; max_local outside 1 .. SLAM_LOCAL_MAXLM; open while open; cnt < 0 or > max_local; an id
 *                    outside 1 .. N or twice; any per-step call, close or abort while no area is open; a local id of update outside
 *                    1 .. the local landmark count; SLAM_FORM_JOSEPH; close after the global N changed
 *   SLAM_E_CAPACITY  augment: the local landmark count + nn would exceed max_local, or N at open + the landmarks added locally
 *                    + nn would exceed the capacity of the global handle
 *
 * info[8]: [0] an area is open  [1] n0  [2] n_a  [3] landmarks added locally  [4] per-step calls since open  [5] N at open
 *          [6] max_local  [7] 0.   While no area is open [1] .. [5] describe the last one (0 before the first).
 * get: phi (n_a x n0), psi (n0 x n0), theta (n0) as doubles, ROW-major and dense; any of the three may be NULL.
 */
#ifndef SLAMHIP_LOCAL_H
#define SLAMHIP_LOCAL_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_LOCAL_MAXLM 1024

typedef struct slam_ekf_local* slam_ekf_local_t;

int slam_ekf_local_create(slam_ekf_local_t* out, slam_ekf_t global, int max_local);

int slam_ekf_local_destroy(slam_ekf_local_t L);

int slam_ekf_local_open(slam_ekf_local_t L, const int32_t* ids, int cnt);

int slam_ekf_local_state(slam_ekf_local_t L, slam_ekf_t* local);

int slam_ekf_local_predict(slam_ekf_local_t L, double v, double g, double wheelbase, const double* Q, double dt);

int slam_ekf_local_update(slam_ekf_local_t L, const double* z, const int32_t* idf_local, int m, const double* R, int form);

int slam_ekf_local_augment(slam_ekf_local_t L, const double* zn, int nn, const double* R);

int slam_ekf_local_close(slam_ekf_local_t L, int* first_new);

int slam_ekf_local_abort(slam_ekf_local_t L);

int slam_ekf_local_info(slam_ekf_local_t L, int64_t* out);

int slam_ekf_local_get(slam_ekf_local_t L, double* phi, double* psi, double* theta);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_LOCAL_H */
