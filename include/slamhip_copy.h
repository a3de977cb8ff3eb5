/* slamhip_copy.h -- an EKF state moved between two handles on the device: copied, grown into a larger capacity, or a sub-map
 * taken out of it.  The entry points of the COMPANION library libslamhip_copy.so.  The reference re-allocates where a map
 * outgrows its matrix (src/ekf.jl:108-109); a handle's capacity is fixed, so the state moves into a larger handle instead.
 *
 * A library of its own for the reason slamhip_frame.h gives: libslamhip.so exports exactly what slamhip.h and slamhip_diag.h
 * declare.  libslamhip_copy.so is built from csrc/ekf_copy.hip by the same Makefile, links against libslamhip.so (it works on
 * that library's handles and calls its internal helpers: both come from one tree and one make) and is found beside it.  Same
 * conventions: extern "C", int status codes, slam_last_error() of libslamhip.so carries the message.
 *
 * WHY A KERNEL.  The covariance is stored tile-major, block lower (slam_ekf_device_ptrs): tile (I, J), I >= J, of edge E (128
 * fp32, 64 fp64) is block number J T - J (J - 1) / 2 + (I - J) with T = ld / E the tile rows of the ALLOCATION.  Two handles of
 * different capacity hold the same matrix at different offsets: a memcpy of the buffer is right between equal ld only.
 *
 * THE RULE (tests/copy_ref.py runs it literally).  n' = 3 + 2 N' is the state dst receives, n_old the one it held, and
 *     s(i) = i                                     for i < 3 and for a copy
 *     s(i) = 3 + 2 (ids[(i - 3) / 2] - 1) + ((i - 3) & 1)   for a select: dst's landmark k is src's landmark ids[k - 1]
 * the source state index of destination index i.  Then x'[i] = x[s(i)], P'[i, j] = P[s(i), s(j)]: a selection of rows and
 * columns, which is what the marginal of a Gaussian is.  Bits are copied; no arithmetic is done on any value.
 *   Tw = min(T_dst, ceil(max(n_old, n') / E)) tile rows of dst are written: every tile (I, J), J <= I < Tw, completely -- with
 *   the selected values where row and column are below n', with +0.0 elsewhere, so what a larger state left behind is padding
 *   again.  Tiles with I >= Tw held padding before and are not touched.
 * Work items are (tile q, slice u): q = 0 .. Tw (Tw + 1) / 2 - 1 numbers the tiles band after band as if Tw were the
 * allocation (J = the band with base(J) <= q < base(J + 1), base(J) = J Tw - J (J - 1) / 2; I = J + q - base(J)), u numbers
 * the E / 32 slices of 32 columns (16 KiB).  Workgroup b of a grid of G <= 2048 takes the items b, b + G, b + 2 G, ...
 *   copy:    a tile with I < ceil(n' / E) is src's tile (I, J) as it is stored (its rows and columns >= n' are +0.0 in src: the
 *            storage invariant), any other tile is zeros.  Thread t of 256 owns the 16-byte pieces t, t + 256, t + 512, t + 768 of
 *            the slice: 16-byte loads and stores, tile bases 32 / 64 KiB aligned on both sides.
 *   select:  thread t owns the entries (row rl = t mod E, columns cl = 32 u + t / E + k (256 / E), k = 0 .. 32 E / 256 - 1) of the
 *            slice: the lanes of a wave walk the ROWS of one destination column, so stores are coalesced and the source column
 *            s(c') is the same for the whole wave.  Below the diagonal tiles it stores its entry at p_off(r', c').  Inside a
 *            diagonal tile the thread with r' >= c' owns the entry AND its mirror and writes both from the one value it loaded
 *            (p_store_sym); a thread with r' < c' writes nothing.
 *            A source entry (a, b) = (s(r'), s(c')) is read from where it is stored: p_off(a, b) when a's tile row >= b's,
 *            p_off(b, a) otherwise; when both lie in one source diagonal tile the LOWER entry p_off(max, min) is read (the
 *            convention of slam_ekf_state_written).  Every entry goes through p_off of its own matrix, so a landmark whose two
 *            rows straddle a tile edge in src, in dst or in both needs nothing special.
 * Every stored offset of dst below Tw is therefore written exactly once (an entry and its mirror by one thread), nothing else
 * is.  All offsets are 64-bit (N = 50000 fp64: 5e9 elements).  No LDS, no atomics, nothing is allocated per call; select
 * sends ids through dst's pinned observation staging and its device index buffer, which grow only.
 *
 * dst AFTERWARDS: N', x[0 : n'), P as above; x beyond n' is left as it was (slam_ekf_set_state does the same); the packed
 * 2 x 2 side array is rebuilt from the matrix; the panel workspace is zeroed when N shrinks; the pre-gate's variance bound
 * and the grid are marked stale.  Gate mode, async flag, timing and update workspace stay dst's own.  src is never written.
 *
 * Decided before anything is enqueued, both states unchanged bit for bit:
 *   SLAM_E_BADARG    a null handle, dst == src, different dtypes, different devices, cnt < 0, ids null with cnt > 0, an id
 *                    outside 1 .. N_src, a repeated id
 *   SLAM_E_CAPACITY  the result (N_src, or cnt) exceeds dst's capacity
 * SLAM_E_HIP from the runtime once work has been enqueued: if a launch failed, dst's state is undefined (upload it again); if
 * only the event that orders src behind the call failed, dst is complete and src must be synchronised with dst before it is written.
 * Ordering, as slam_ekf_join: src's deferred asynchronous status is resolved first, as slam_ekf_sync(src) would (an error of src
 * is returned, dst is untouched).  The work is enqueued on dst's stream behind everything enqueued there and behind an event
 * recorded on src's stream; an event recorded on dst's stream after the last read of src is made a dependency of src's stream,
 * so src may be updated or destroyed as soon as the call returns.  Enqueued, does not synchronise. */
#ifndef SLAMHIP_COPY_H
#define SLAMHIP_COPY_H

#include "slamhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The landmark capacity the handle was created with. */
int slam_ekf_capacity(slam_ekf_t h, int* max_landmarks);

/* dst <- src: N, x[0 : n), every entry of P, bit for bit.  The capacities may differ in either direction as long as
 * N_src <= dst's capacity.  Equal ld runs the same kernel with equal block numbers. */
int slam_ekf_copy(slam_ekf_t dst, slam_ekf_t src);

/* dst <- the marginal of src over the vehicle and the landmarks ids[0 .. cnt): 1-based, distinct, in any order; cnt = 0 gives the
 * vehicle alone.  dst's landmark k is src's landmark ids[k - 1]. */
int slam_ekf_select(slam_ekf_t dst, slam_ekf_t src, const int32_t* ids, int cnt);

#ifdef __cplusplus
}
#endif

#endif /* SLAMHIP_COPY_H */
