"""Dense fp64 NumPy restatement of the rule of include/ext/slamhip_iterated.h: the iterated EKF update (Gauss-Newton on the MAP
cost of one batch of range-bearing observations, no line search), in its REDUCED form over the 3 + 2m states H touches -- what the
kernel runs -- and in the full n-dimensional form it must equal.  Ids are 1-based, z is 2 x m (range; bearing), R is 2 x 2.

tests/test_iterated_ref_cpu.py pins this file against the oracle's update and against itself; tests/test_gpu_ekf_iterated.py
compares the kernels with it.  The designed hard scenes of both live here."""
import math

import numpy as np

from oracle import ekf_ref as O
from tests.linear_ref import chol_lower, f

MAXOBS = 8
MAXITER = 64
R_HARD = np.diag([0.05 ** 2, (0.5 * math.pi / 180) ** 2])


def state_indices(idf):
    """a: 0, 1, 2 and the two indices of every id in the order given, duplicates kept."""
    a = [0, 1, 2]
    for j in np.asarray(idf).reshape(-1):
        a += [f(j), f(j) + 1]
    return np.array(a, dtype=np.int64)


def model(xa, z):
    """(r [2m], H [2m, 3 + 2m]) at the reduced iterate xa: observation k sees the landmark at xa[3 + 2k : 5 + 2k]."""
    m = z.shape[1]
    ids = np.arange(1, m + 1)
    zp, Hv, Hf = O.obs_blocks(xa, ids)
    H = np.zeros((2 * m, 3 + 2 * m))
    r = np.empty(2 * m)
    for k in range(m):
        H[2 * k:2 * k + 2, 0:3] = Hv[k]
        H[2 * k:2 * k + 2, 3 + 2 * k:5 + 2 * k] = Hf[k]
        r[2 * k] = z[0, k] - zp[k, 0]
        r[2 * k + 1] = O.mpi_to_pi(z[1, k] - zp[k, 1])
    return r, H


def cost_terms(r, R):
    """sum_k r_k' inv(R) r_k."""
    Ri = np.linalg.inv(R)
    return float(sum(r[2 * k:2 * k + 2] @ Ri @ r[2 * k:2 * k + 2] for k in range(len(r) // 2)))


def iterate(x0a, Pa, z, R, max_iter, tol):
    """The loop of the header on the reduced block.  Returns (out[10], pieces, steps): pieces = (H, C, g) of the last iteration, or
    None after a failing pivot; steps = every step_i."""
    x0a = np.asarray(x0a, dtype=np.float64)
    Pa = np.asarray(Pa, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    R = np.asarray(R, dtype=np.float64)
    m = z.shape[1]
    RR = np.kron(np.eye(m), R)
    xi = x0a.copy()
    steps = []
    it, step, jfirst, jlast = 0, 0.0, 0.0, 0.0
    while True:
        r, H = model(xi, z)
        v = r - H @ (x0a - xi)
        PaHt = Pa @ H.T
        S = H @ PaHt + RR
        S = (S + S.T) * 0.5
        Lf, j, d = chol_lower(S)
        if j >= 0:
            return np.array([it, 0.0, step, 0.0, 0.0, d, j, it, jfirst, jlast], dtype=np.float64), None, steps
        Li = np.linalg.inv(Lf)
        y = Li @ v
        g = Li.T @ y
        xn = x0a + PaHt @ g
        step = float(np.max(np.abs(xn - xi)))
        steps.append(step)
        jlast = float(g @ (S - RR) @ g) + cost_terms(model(xn, z)[0], R)
        if it == 0:
            jfirst = jlast
        it += 1
        conv = step <= tol
        if conv or it == max_iter:
            out = np.array([it, 1.0 if conv else 0.0, step, float(y @ y), 2.0 * float(np.sum(np.log(np.diag(Lf)))),
                            float(np.min(np.diag(Lf))), -1.0, -1.0, jfirst, jlast])
            return out, (H, Li.T, g), steps
        xi = xn


def update(x, P, z, R, idf, max_iter=10, tol=1e-9, with_steps=False):
    """(x, P, out) after slam_ekf_update_iterated; x and P come back unchanged (copies) after a failing pivot (out[6] >= 0)."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    a = state_indices(idf)
    assert 1 <= z.shape[1] <= MAXOBS and len(a) == 3 + 2 * z.shape[1]
    out, pieces, steps = iterate(x[a], P[np.ix_(a, a)], z, R, max_iter, tol)
    if pieces is None:
        res = (x.copy(), P.copy(), out)
    else:
        H, C, g = pieces
        PHt = P[:, a] @ H.T                                 # P H' with H scattered into the columns a (duplicates add up)
        W1 = PHt @ C
        res = (x + PHt @ g, P - W1 @ W1.T, out)
    return res + (steps,) if with_steps else res


def update_batches(x, P, z, R, idf, max_iter=10, tol=1e-9):
    """More than MAXOBS observations: consecutive batches of MAXOBS in the order given, each on the state the batch before left.
    Returns (x, P, [out of every batch])."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    idf = np.asarray(idf).reshape(-1)
    outs = []
    for s in range(0, z.shape[1], MAXOBS):
        x, P, out = update(x, P, z[:, s:s + MAXOBS], R, idf[s:s + MAXOBS], max_iter, tol)
        outs.append(out)
    return x, P, outs


def full_H(x, z, idf):
    """(r, H [2m, n]) of the dense model at the full state x (oracle.ekf_ref.predict_observation, row pair by row pair)."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    m = z.shape[1]
    H = np.zeros((2 * m, len(x)))
    r = np.empty(2 * m)
    for k, j in enumerate(np.asarray(idf).reshape(-1)):
        zp, Hk = O.predict_observation(x, j)
        H[2 * k:2 * k + 2] = Hk
        r[2 * k] = z[0, k] - zp[0]
        r[2 * k + 1] = O.mpi_to_pi(z[1, k] - zp[1])
    return r, H


def update_full(x, P, z, R, idf, max_iter=10, tol=1e-9):
    """The same iteration on all n states with the dense n-column H: what the reduced form must reproduce.  The stop looks at the
    states in a, as the reduced form does (no other state's step is larger: they move through P[:, a] only -- but the rule is the
    rule).  Returns (x, P, iterations)."""
    x0 = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    RR = np.kron(np.eye(z.shape[1]), np.asarray(R, dtype=np.float64))
    a = state_indices(idf)
    xi = x0.copy()
    it = 0
    while True:
        r, H = full_H(xi, z, idf)
        v = r - H @ (x0 - xi)
        PHt = P @ H.T
        S = H @ PHt + RR
        S = (S + S.T) * 0.5
        C = np.linalg.inv(np.linalg.cholesky(S)).T
        g = C @ (C.T @ v)
        xn = x0 + PHt @ g
        step = float(np.max(np.abs(xn[a] - xi[a])))
        it += 1
        if step <= tol or it == max_iter:
            W1 = PHt @ C
            return xn, P - W1 @ W1.T, it
        xi = xn


def map_cost(xa, x0a, Pa, z, R):
    """J at a reduced point: (xa - x0a)' inv(Pa) (xa - x0a) + sum_k r_k' inv(R) r_k (distinct ids only: Pa is then invertible)."""
    d = np.asarray(xa, dtype=np.float64) - x0a
    return float(d @ np.linalg.solve(Pa, d)) + cost_terms(model(xa, np.asarray(z, dtype=np.float64).reshape(2, -1))[0], R)


def cost_gradient(xa, x0a, Pa, z, R, h=1e-6):
    """Central differences of map_cost."""
    grad = np.zeros(len(xa))
    for q in range(len(xa)):
        e = np.zeros(len(xa))
        e[q] = h
        grad[q] = (map_cost(xa + e, x0a, Pa, z, R) - map_cost(xa - e, x0a, Pa, z, R)) / (2 * h)
    return grad


# ---- the designed hard scenes -------------------------------------------------------------------------------------------------------
def harden(x, P, ids, seed, heading=None, across_cut=False):
    """A hard scene on the state (x, P), returned as (x, P, z): the observed landmarks ids (1-based; one named twice is observed
    twice) are moved to 3 .. 10 m from the vehicle, the vehicle block of P is inflated to (0.5 m)^2, (0.5 m)^2, (0.2 rad)^2 with its
    cross-covariances to the map cleared, and z is what a sensor of noise R_HARD sees from a TRUE pose drawn 0.5 .. 0.9 sigma from the
    prior mean on every axis: one linearisation at the prior mean is then visibly not enough.  across_cut: the first bearing is
    reported on the other side of the +-pi cut from the prediction at the prior mean, so that z - zp is 2 pi off before the wrap."""
    rng = np.random.default_rng(seed)
    x = np.array(x, dtype=np.float64)
    P = np.array(P, dtype=np.float64)
    if heading is not None:
        x[2] = heading
    ids = np.asarray(ids).reshape(-1)
    m = len(ids)
    ang = rng.uniform(-math.pi, math.pi, m)
    dist = rng.uniform(3.0, 10.0, m)
    for k, j in enumerate(ids):
        x[f(j)] = x[0] + dist[k] * math.cos(ang[k])
        x[f(j) + 1] = x[1] + dist[k] * math.sin(ang[k])
    P[0:3, :] = 0.0
    P[:, 0:3] = 0.0
    P[0, 0] = P[1, 1] = 0.5 ** 2
    P[2, 2] = 0.2 ** 2
    truth = x.copy()
    truth[0:3] += rng.choice([-1.0, 1.0], 3) * rng.uniform(0.5, 0.9, 3) * np.array([0.5, 0.5, 0.2])
    z = np.zeros((2, m))
    for k, j in enumerate(ids):
        zp = O.predict_observation(truth, j)[0]
        z[:, k] = [zp[0] + rng.normal(0, 0.05), O.mpi_to_pi(zp[1]) + rng.normal(0, 0.5 * math.pi / 180)]
    if across_cut:                                          # z - zp at the prior mean is 2 pi off: the one wrap of the rule is needed
        d = z[1, 0] - O.predict_observation(x, ids[0])[0][1]
        if abs(d) <= math.pi:
            z[1, 0] += 2 * math.pi if d < 0 else -2 * math.pi
    return x, P, z


CAP = 256
STRADDLER = {"f32": 63, "f64": 31}                          # the landmark whose pair straddles a tile edge (128 / 64)
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
TOL_HARD, ITER_HARD = 1e-9, 20


def base_state(N, dtype):
    """The designed `slam` state of the record tests (tests/update_records.py) for N >= 70; a small dense one below."""
    if N >= 70:
        from tests import update_records as UR
        x, P = UR.designed_state("slam", N, dtype, 1000 + N)
        return np.array(x), np.array(P)
    rng = np.random.default_rng(40 + N)
    n = 3 + 2 * N
    x = np.concatenate([[3.0, -2.0, 0.4], rng.uniform(-20, 20, 2 * N)])
    A = rng.normal(0, 0.3, (n, n))
    P = A @ A.T + 0.05 * np.eye(n)
    return x, (P + P.T) / 2


# name -> (N, ids with s for the straddler, seed per dtype, heading, across the cut).  The seeds are chosen so that the conditions
# of tests/test_iterated_ref_cpu.py hold: the reference converges within ITER_HARD iterations at TOL_HARD and no step lies within
# a factor 4 of TOL_HARD.
SCENES = {
    "N1-m1": (1, [1], {"f64": 80, "f32": 80}, None, False),
    "N70-m3-straddler": (70, ["s", 70, 12], {"f64": 3, "f32": 2}, None, False),
    "N70-m8": (70, ["s", 70, 1, 12, 45, 33, 64, 5], {"f64": 33, "f32": 6}, None, False),
    "N200-m8-last": (200, [200, "s", 120, 7, 64, 65, 150, 99], {"f64": 3, "f32": 3}, None, False),
    "N200-m3-duplicate": (200, ["s", 200, "s"], {"f64": 3, "f32": 11}, None, False),
    "N70-m3-cut": (70, [70, "s", 9], {"f64": 2, "f32": 3}, 3.1, True),
    "N200-m11": (200, [200, "s", 120, 7, 64, 65, 150, 99, 3, 181, 42], {"f64": 24, "f32": 6}, None, False),
}


def scene(name, dtype, seed=None):
    """(x, P, z, ids) of a hard scene; x and P hold values of the dtype exactly, so an upload changes nothing."""
    N, ids, seeds, heading, cut = SCENES[name]
    ids = np.array([STRADDLER[dtype] if j == "s" else j for j in ids], dtype=np.int64)
    x, P = base_state(N, dtype)
    x, P, z = harden(x, P, ids, seeds[dtype] if seed is None else seed, heading, cut)
    t = NP_DTYPE[dtype]
    return x.astype(t).astype(np.float64), P.astype(t).astype(np.float64), z, ids


def steps_clear_of(steps, tol, factor=4.0):
    """No step within `factor` of tol: an ulp of difference in the device's trigonometry cannot change the iteration count."""
    return all(s > factor * tol or s < tol / factor for s in steps)
