"""What the gating keeps beside x and P (csrc/common.h, struct slam_ekf: the packed diagonal blocks, the variance bound `pmax`, the
grid over the landmark means) decides which landmarks an observation is compared with at all.  This file restates, in NumPy
float64 and from the comments and code of csrc/ekf_gate.hip, the two reaches that are derived from the bound -- the sweep's
pre-gate (pre_gate()) and the grid query's annulus and sector (gate_grid_kernel) -- so that a test scene can be shown to be one
where a STALE bound or a STALE grid item would take another decision than the exact gate.  Host-only.

All functions take the state in float64 as the device holds it; landmark ids are 1-based."""
import math

import numpy as np

SLACK = 1.0 + 1e-6          # pre_gate(): `slack`; gate_grid_kernel: the factor on rho and beta
ABS = 1e-9                  # gate_grid_kernel: the absolute term on rho and beta


def f(j):
    """State index of landmark j (1-based)."""
    return 3 + 2 * (int(j) - 1)


def mpi_to_pi(a):
    return math.remainder(a, 2.0 * math.pi)


def true_pmax(P):
    """max diag(P[3:, 3:]): the smallest value the device's bound may hold (0 without a landmark)."""
    d = np.diag(np.asarray(P, dtype=np.float64))[3:]
    return float(d.max()) if d.size else 0.0


def innovation(x, z, j):
    """(v0, v1, d): range and wrapped bearing innovation of observation z against landmark j, and the distance pose -> landmark."""
    dx, dy = x[f(j)] - x[0], x[f(j) + 1] - x[1]
    d = math.hypot(dx, dy)
    return z[0] - d, mpi_to_pi(z[1] - (math.atan2(dy, dx) - x[2])), d


def pre_gate_bounds(x, P, j, pmax, R, gate2):
    """(b0, b1) of pre_gate() for landmark j: gate2 * B_k * slack, +inf where the bound is not usable.  The sweep skips the pair
    (observation, j) when v_0^2 > b0 or v_1^2 > b1."""
    x, P, R = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64), np.asarray(R, dtype=np.float64)
    dx, dy = x[f(j)] - x[0], x[f(j) + 1] - x[1]
    d2 = dx * dx + dy * dy
    d = math.sqrt(d2)
    sx, sy, sp, sm = math.sqrt(P[0, 0]), math.sqrt(P[1, 1]), math.sqrt(P[2, 2]), math.sqrt(pmax)
    ax, ay = abs(dx), abs(dy)
    with np.errstate(all="ignore"):
        a0 = np.float64(ax * sx + ay * sy + (ax + ay) * sm) / np.float64(d)
        a1 = np.float64(ay * sx + ax * sy + (ax + ay) * sm) / np.float64(d2) + sp
        b0 = float(gate2 * (a0 * a0 + R[0, 0]) * SLACK)
        b1 = float(gate2 * (a1 * a1 + R[1, 1]) * SLACK)
    if not (b0 > 0.0 and b0 < math.inf):
        b0 = math.inf
    if not (b1 > 0.0 and b1 < math.inf):
        b1 = math.inf
    return b0, b1


def grid_reach(x, P, z, pmax, R, gate2):
    """The reach of observation z = (r, b) in the grid form (ekf_gate.hip, "N2, the O(candidates) form"): a dict with `rho`,
    `beta` (pi: the whole annulus) and the annulus `lo`, `hi` = [max(r - rho, 0), r + rho] of distances pose -> landmark mean that can
    matter, before the query widens it by the recorded drift."""
    x, P, R = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64), np.asarray(R, dtype=np.float64)
    A0 = math.sqrt(max(P[0, 0], 0.0) + max(P[1, 1], 0.0)) + math.sqrt(2.0 * max(pmax, 0.0))
    sp = math.sqrt(max(P[2, 2], 0.0))
    rho = math.sqrt(gate2 * (A0 * A0 + R[0, 0])) * SLACK + ABS
    lo, hi = max(z[0] - rho, 0.0), z[0] + rho
    beta = math.pi
    if lo > 0.0:
        a1 = A0 / lo + sp
        beta = min(math.pi, math.sqrt(gate2 * (a1 * a1 + R[1, 1])) * SLACK + ABS)
    return {"rho": rho, "beta": beta, "lo": lo, "hi": hi}


def annulus_ratio(pose, mean, z, reach):
    """|distance pose -> mean minus the observed range| over rho: above 1 the mean lies outside the annulus."""
    return abs(math.hypot(mean[0] - pose[0], mean[1] - pose[1]) - z[0]) / reach["rho"]


def stale_would_miss(x, P, z, j, R, gate2, pmax_old, x_old=None, recomputed=False):
    """For one (observation z, landmark j) pair of the state (x, P) AFTER a call, which the exact gate accepts: how far would the
    side state of BEFORE the call be from finding it?  Returns the ratios (each > 1 means "missed"; the tests ask for >= 2):
      a  max_k v_k^2 / (gate2 B_k), B_k from the OLD bound pmax_old: the sweep's pre-gate would skip the pair;
      b  |d - r| / rho with rho from the OLD bound and d the landmark's CURRENT mean: a grid rebuilt from the new means but
         queried under the old bound would leave it outside the annulus;
      c  |d_old - r| / rho with rho from the NEW bound, no recorded drift, and d_old the mean that a grid item of index j carried
         BEFORE the call (x_old; None, or an index the old map did not have: nan -- an appended landmark is read from the tail,
         not from an item).  The new bound is true_pmax(P) where the call makes the device recompute it (`recomputed`), else the
         larger of that and the old one: a down-date never lowers the device's bound, add_features raises it."""
    x, P = np.asarray(x, dtype=np.float64), np.asarray(P, dtype=np.float64)
    v0, v1, _d = innovation(x, z, j)
    b0, b1 = pre_gate_bounds(x, P, j, pmax_old, R, gate2)
    a = max(v0 * v0 / (b0 / SLACK), v1 * v1 / (b1 / SLACK))
    b = annulus_ratio(x[0:2], x[f(j):f(j) + 2], z, grid_reach(x, P, z, pmax_old, R, gate2))
    c = math.nan
    if x_old is not None and f(j) + 2 <= len(x_old):
        new = grid_reach(x, P, z, true_pmax(P) if recomputed else max(pmax_old, true_pmax(P)), R, gate2)
        c = annulus_ratio(x[0:2], np.asarray(x_old, dtype=np.float64)[f(j):f(j) + 2], z, new)
    return {"a": float(a), "b": float(b), "c": float(c)}


def evaluated_bounds(x, P, z, built, pmax, R, gate2, drift=0.0):
    """(least, most): how many landmarks a grid query evaluates for observation z when the bound it reads is `pmax`, the items
    carry the means `built` ([2 N], as x[3:]) and the recorded drift is `drift` (gate_grid_kernel).  most: every item inside the
    annulus widened by sqrt(2) drift (the cells of the sector's bounding box can only leave some of them out); least: the items
    inside the plain annulus AND inside the sector, which lie in that bounding box whatever the cells are."""
    x = np.asarray(x, dtype=np.float64)
    reach = grid_reach(x, P, z, pmax, R, gate2)
    b = np.asarray(built, dtype=np.float64).reshape(-1, 2)
    dx, dy = b[:, 0] - x[0], b[:, 1] - x[1]
    d = np.hypot(dx, dy)
    pad = math.sqrt(2.0) * drift + 1e-9 * (reach["hi"] + abs(x[0]) + abs(x[1]) + 1.0)
    most = int(np.count_nonzero((d >= reach["lo"] - pad) & (d <= reach["hi"] + pad)))
    ang = np.abs(np.remainder(np.arctan2(dy, dx) - x[2] - z[1] + math.pi, 2.0 * math.pi) - math.pi)
    least = int(np.count_nonzero((d >= reach["lo"]) & (d <= reach["hi"]) & (ang <= reach["beta"])))
    return least, most
