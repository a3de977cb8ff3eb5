"""Dense fp64 NumPy restatement of the rule of include/ext/slamhip_fej.h: the first-estimates Jacobian (FEJ) predict, update and
augment of 2-D range-bearing EKF-SLAM.  No formula of the filter changes, only where its Jacobians are evaluated: every landmark
at its FIRST estimate (`first`), the vehicle at its PREDICTED pose (`lin`), never at an updated one.  A state is the four arrays
(x, P, lin, first); ids are 1-based, z is 2 x m (range; bearing), R and Q are 2 x 2.

`rnd` is the rounding of a stored entry (identity: an fp64 state; np.float32: an fp32 one): the rule uses the new pose and a new
landmark's mean AS STORED where it forms a Jacobian from them, so that the three directions below are kept to the last bit.

Also here: the twin that re-sets lin / first to the current estimates before every call (the standard filter, i.e. the oracle),
the matrix N of the three unobservable directions and how a filter's own Jacobians carry it forward, and drive(), the seeded
10-landmark run that tests/test_fej_ref_cpu.py and tests/test_gpu_ekf_fej.py chain."""
import math

import numpy as np

from oracle import ekf_ref as O
from tests.linear_ref import chol_lower, f

MAXOBS = 8
J2 = np.array([[0.0, -1.0], [1.0, 0.0]])
R_DRIVE = np.diag([0.1 ** 2, (math.pi / 180) ** 2])
X0_DRIVE = np.array([1.0, -2.0, 0.4])
P0_DRIVE = np.diag([0.04, 0.04, 0.01])
Q_DRIVE = np.diag([0.3 ** 2, (3 * math.pi / 180) ** 2])
WHEELBASE, DT, OBS_EVERY, SENSOR_RANGE = 4.0, 0.1, 8, 30.0


def ident(a):
    return a


def create(x):
    """(lin, first) of a fresh object: the stored pose and the stored landmark means."""
    x = np.asarray(x, dtype=np.float64)
    return x[0:3].copy(), x[3:].copy()


# ---- the rule --------------------------------------------------------------------------------------------------------------------
def predict(x, P, lin, first, v, g, w, Q, dt, rnd=ident):
    """src/ekf.jl:8-43 with Gv's third column J (x+[0:2] - lin[0:2]) in place of J (x+[0:2] - x[0:2]).  Returns new
    (x, P, lin, first) and the Gv used."""
    x = np.array(x, dtype=np.float64)
    P = np.array(P, dtype=np.float64)
    phi = x[2]
    s, c = math.sin(g + phi), math.cos(g + phi)
    vts, vtc = v * dt * s, v * dt * c
    xp = np.array([rnd(x[0] + vtc), rnd(x[1] + vts), rnd(O.mpi_to_pi(phi + v * dt * math.sin(g) / w))], dtype=np.float64)
    Gv = np.eye(3)
    Gv[0:2, 2] = J2 @ (xp[0:2] - lin[0:2])
    Gu = np.array([[dt * c, -vts], [dt * s, vtc], [dt * math.sin(g) / w, v * dt * math.cos(g) / w]])
    P[0:3, 0:3] = Gv @ P[0:3, 0:3] @ Gv.T + Gu @ np.asarray(Q, dtype=np.float64) @ Gu.T
    if P.shape[0] > 3:
        P[0:3, 3:] = Gv @ P[0:3, 3:]
        P[3:, 0:3] = P[0:3, 3:].T
    x[0:3] = xp
    return x, P, xp.copy(), np.array(first, dtype=np.float64), Gv


def jacobian_blocks(lin, first, idf):
    """(Hv [m, 2, 3], Hf [m, 2, 2]) of src/common.jl:139-165 at the pose lin and the landmarks first[idf]."""
    _, Hv, Hf = O.obs_blocks(np.concatenate([lin, first]), idf)
    return Hv, Hf


def dense_H(lin, first, idf, n):
    idf = np.asarray(idf).reshape(-1)
    Hv, Hf = jacobian_blocks(lin, first, idf)
    H = np.zeros((2 * len(idf), n))
    for k, j in enumerate(idf):
        H[2 * k:2 * k + 2, 0:3] = Hv[k]
        H[2 * k:2 * k + 2, f(j):f(j) + 2] = Hf[k]
    return H


def update(x, P, lin, first, z, R, idf):
    """The residuals at x, the Jacobian at (lin, first), then the reference's Cholesky form.  Returns (x, P, out[4], H); x and P
    come back unchanged (copies) after a failing pivot (out[3] >= 0).  lin and first are not changed."""
    x = np.asarray(x, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    idf = np.asarray(idf).reshape(-1)
    m = z.shape[1]
    assert 1 <= m <= MAXOBS and len(idf) == m
    zp = O.obs_blocks(x, idf)[0]
    r = np.empty(2 * m)
    r[0::2] = z[0] - zp[:, 0]
    r[1::2] = [O.mpi_to_pi(a) for a in z[1] - zp[:, 1]]
    with np.errstate(all="ignore"):
        H = dense_H(lin, first, idf, len(x))
        PHt = P @ H.T
        S = H @ PHt + np.kron(np.eye(m), np.asarray(R, dtype=np.float64))
        S = (S + S.T) * 0.5
    Lf, j, d = chol_lower(S)
    if j >= 0:
        return x.copy(), P.copy(), np.array([0.0, 0.0, d, float(j)]), H
    Li = np.linalg.inv(Lf)
    y = Li @ r
    g = Li.T @ y
    W1 = PHt @ Li.T
    out = np.array([float(y @ y), 2.0 * float(np.sum(np.log(np.diag(Lf)))), float(np.min(np.diag(Lf))), -1.0])
    return x + PHt @ g, P - W1 @ W1.T, out, H


def update_batches(x, P, lin, first, z, R, idf):
    """More than MAXOBS observations: consecutive batches of MAXOBS.  The Jacobians do not move between the batches; the residuals
    of a batch are taken at the mean the batch before left.  Returns (x, P, [out of every batch])."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    idf = np.asarray(idf).reshape(-1)
    outs = []
    for s in range(0, z.shape[1], MAXOBS):
        x, P, out, _ = update(x, P, lin, first, z[:, s:s + MAXOBS], R, idf[s:s + MAXOBS])
        outs.append(out)
    return x, P, outs


def add_features(x, P, lin, first, z, R, rnd=ident):
    """src/ekf.jl:84-122 with Gv = [I | J (lm - lin[0:2])], lm the new mean as stored.  Returns new (x, P, lin, first) and the
    list of the Gv used."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    x = np.array(x, dtype=np.float64)
    P = np.array(P, dtype=np.float64)
    first = np.array(first, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    phi = x[2]
    used = []
    for i in range(z.shape[1]):
        ln = len(x)
        r, b = z[0, i], z[1, i]
        s, c = math.sin(phi + b), math.cos(phi + b)
        lm = np.array([rnd(x[0] + r * c), rnd(x[1] + r * s)], dtype=np.float64)
        Gv = np.hstack([np.eye(2), (J2 @ (lm - lin[0:2])).reshape(2, 1)])
        Gz = np.array([[c, -r * s], [s, r * c]])
        Pn = np.zeros((ln + 2, ln + 2))
        Pn[:ln, :ln] = P
        P = Pn
        rng = slice(ln, ln + 2)
        P[rng, rng] = Gv @ P[0:3, 0:3] @ Gv.T + Gz @ R @ Gz.T
        P[rng, 0:ln] = Gv @ P[0:3, 0:ln]
        P[0:ln, rng] = P[rng, 0:ln].T
        x = np.concatenate([x, lm])
        first = np.concatenate([first, lm])
        used.append(Gv)
    return x, P, np.array(lin, dtype=np.float64), first, used


def reset(x, lin, first, ids=None, pose=False):
    """first of the listed landmarks (None: all) <- their stored means; with pose, lin <- the stored pose."""
    lin, first = np.array(lin, dtype=np.float64), np.array(first, dtype=np.float64)
    ids = np.arange(1, len(first) // 2 + 1) if ids is None else np.asarray(ids).reshape(-1)
    for j in ids:
        first[f(j) - 3:f(j) - 1] = x[f(j):f(j) + 2]
    if pose:
        lin = np.array(x[0:3], dtype=np.float64)
    return lin, first


def remap(x, first, ids):
    """After the map was renumbered outside: new landmark j takes the first estimate of old landmark ids[j - 1] (1-based), or the
    current stored mean where ids[j - 1] == 0.  x is the renumbered state."""
    ids = np.asarray(ids).reshape(-1)
    assert 3 + 2 * len(ids) == len(x)
    new = np.empty(2 * len(ids))
    for j, o in enumerate(ids):
        assert 0 <= o <= len(first) // 2
        new[2 * j:2 * j + 2] = x[3 + 2 * j:5 + 2 * j] if o == 0 else first[2 * (o - 1):2 * o]
    return new


def transform(lin, first, tx, ty, theta):
    """The map of include/slamhip_frame.h for the means, applied to lin and every first estimate."""
    theta = math.remainder(theta, 2.0 * math.pi)
    c, s = math.cos(theta), math.sin(theta)
    Rm = np.array([[c, -s], [s, c]])
    nl = np.concatenate([Rm @ lin[0:2] + [tx, ty], [O.mpi_to_pi(lin[2] + theta)]])
    nf = (np.asarray(first).reshape(-1, 2) @ Rm.T + [tx, ty]).reshape(-1)
    return nl, nf


def transform_state(x, P, tx, ty, theta):
    """The same frame change of a whole state (x, P): what slam_ekf_transform does."""
    theta = math.remainder(theta, 2.0 * math.pi)
    c, s = math.cos(theta), math.sin(theta)
    Rm = np.array([[c, -s], [s, c]])
    n = len(x)
    T = np.eye(n)
    T[0:2, 0:2] = Rm
    for q in range(3, n, 2):
        T[q:q + 2, q:q + 2] = Rm
    xn = T @ x
    xn[0:2] += [tx, ty]
    xn[3::2] += tx
    xn[4::2] += ty
    xn[2] = O.mpi_to_pi(x[2] + theta)
    return xn, T @ P @ T.T


# ---- the twin: the linearisation points re-set to the current estimates before every call ----------------------------------------
def twin_predict(x, P, v, g, w, Q, dt):
    lin, first = create(x)
    return predict(x, P, lin, first, v, g, w, Q, dt)


def twin_update(x, P, z, R, idf):
    lin, first = create(x)
    return update(x, P, lin, first, z, R, idf)


def twin_add_features(x, P, z, R):
    lin, first = create(x)
    return add_features(x, P, lin, first, z, R)


# ---- the three unobservable directions -------------------------------------------------------------------------------------------
def N_matrix(lin, first):
    """[3 + 2N, 3]: the two translations and the rotation of the whole map, at the linearisation points."""
    Nl = len(first) // 2
    Nm = np.zeros((3 + 2 * Nl, 3))
    Nm[0:2, 0:2] = np.eye(2)
    Nm[0:2, 2] = J2 @ lin[0:2]
    Nm[2, 2] = 1.0
    for j in range(Nl):
        Nm[3 + 2 * j:5 + 2 * j, 0:2] = np.eye(2)
        Nm[3 + 2 * j:5 + 2 * j, 2] = J2 @ first[2 * j:2 * j + 2]
    return Nm


def carry_predict(Nm, Gv):
    """The directions after a predict whose vehicle Jacobian was Gv."""
    Nm = Nm.copy()
    Nm[0:3] = Gv @ Nm[0:3]
    return Nm


def carry_augment(Nm, Gvs):
    """... after an augment whose new landmarks were entered with the Jacobians Gvs."""
    return np.vstack([Nm] + [G @ Nm[0:3] for G in Gvs])


def information(Nm, P):
    """N' inv(P) N, 3 x 3."""
    return Nm.T @ np.linalg.solve(P, Nm)


def drift(M, M0):
    return float(np.max(np.abs(M - M0)) / np.max(np.abs(M0)))


# ---- the seeded run --------------------------------------------------------------------------------------------------------------
def drive(seed, steps, Q):
    """The calls of a seeded run over 10 landmarks, independent of any filter (the correspondences are known): a list of
    ("predict", v, g, WHEELBASE, Q, DT), ("update", z [2, m <= 8], ids) and ("augment", zn [2, k]).  The vehicle starts at
    X0_DRIVE (the filter: X0_DRIVE with P0_DRIVE) and drives a wide left-hand arc at 3 m/s; the controls the filter is given carry
    noise of covariance Q (none when Q = 0); every OBS_EVERY-th step the sensor (noise R_DRIVE, range SENSOR_RANGE) reports the
    landmarks in range: those seen before as an update of at most 8 (the nearest), the others as new ones."""
    rng = np.random.default_rng(1000 + seed)
    Q = np.asarray(Q, dtype=np.float64)
    ang = rng.uniform(-math.pi, math.pi, 10)
    rad = rng.uniform(8.0, 22.0, 10)
    lms = np.stack([4.0 + rad * np.cos(ang), 6.0 + rad * np.sin(ang)])
    truth = X0_DRIVE.copy()
    seen = {}
    ops = []
    sq = np.sqrt(np.diag(Q))
    for t in range(1, steps + 1):
        v, g = 3.0, 0.12 + 0.05 * math.sin(0.07 * t)
        truth = np.array([truth[0] + v * DT * math.cos(g + truth[2]), truth[1] + v * DT * math.sin(g + truth[2]),
                          O.mpi_to_pi(truth[2] + v * DT * math.sin(g) / WHEELBASE)])
        noise = rng.standard_normal(2) * sq
        ops.append(("predict", v + noise[0], g + noise[1], WHEELBASE, Q, DT))
        if t % OBS_EVERY:
            continue
        d = lms - truth[0:2, None]
        dist = np.hypot(d[0], d[1])
        z = np.stack([dist, np.arctan2(d[1], d[0]) - truth[2]]) + rng.standard_normal((2, 10)) * np.sqrt(np.diag(R_DRIVE))[:, None]
        z[1] = [O.mpi_to_pi(O.mpi_to_pi(a)) for a in z[1]]
        vis = [k for k in np.argsort(dist) if dist[k] < SENSOR_RANGE]
        old = [k for k in vis if k in seen][:MAXOBS]
        new = [k for k in vis if k not in seen]
        if old:
            ops.append(("update", z[:, old], np.array([seen[k] for k in old], dtype=np.int64)))
        if new:
            for k in new:
                seen[k] = len(seen) + 1
            ops.append(("augment", z[:, new]))
    return ops


def run(ops, mode="rule", x=None, P=None):
    """The calls of drive() through the rule ("rule") or its twin ("twin"), from X0_DRIVE / P0_DRIVE.  Returns the list of records
    (op name, x, P, lin, first, N carried forward by the Jacobians used, H of an update or None) after every call, led by the
    record of the start."""
    x = X0_DRIVE.copy() if x is None else np.array(x, dtype=np.float64)
    P = P0_DRIVE.copy() if P is None else np.array(P, dtype=np.float64)
    lin, first = create(x)
    Nm = N_matrix(lin, first)
    hist = [("start", x, P, lin, first, Nm, None)]
    for op in ops:
        H = None
        if mode == "twin":
            lin, first = create(x)
        if op[0] == "predict":
            x, P, lin, first, Gv = predict(x, P, lin, first, *op[1:])
            Nm = carry_predict(Nm, Gv)
        elif op[0] == "update":
            x, P, out, H = update(x, P, lin, first, op[1], R_DRIVE, op[2])
            assert out[3] == -1
        else:
            x, P, lin, first, Gvs = add_features(x, P, lin, first, op[1], R_DRIVE)
            Nm = carry_augment(Nm, Gvs)
        hist.append((op[0], x, P, lin, first, Nm, H))
    return hist
