"""The compressed EKF over a local area (include/ext/slamhip_local.h), run literally in NumPy float64 on dense x, P: the rule
the device library is held against.  The local steps are the oracle's predict_sparse / update_sparse / add_features_sparse on
the sub-state; phi, psi, theta and close are this file's own.  Host-only.

The accumulator rules are also available as pure functions of (phi, psi, theta) and the local state they are applied at, so that
a GPU test can hold the device's accumulators against them step by step from the device's OWN local state (which, in fp32,
differs from this file's fp64 trajectory by the product's rounding)."""
import math

import numpy as np

from oracle import ekf_ref as O

MAXLM = 1024
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
V = 2.0 ** -53


def select_indices(ids):
    """State indices of the vehicle and the landmarks ids (1-based, in the order given)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    s = [0, 1, 2]
    for j in ids:
        s += [3 + 2 * (j - 1), 3 + 2 * (j - 1) + 1]
    return np.array(s, dtype=np.int64)


def dense_H(x, idf):
    """The 2m x n Jacobian of the observations of the landmarks idf at x (5 non-zeros a row)."""
    idf = np.asarray(idf, dtype=np.int64).reshape(-1)
    _zp, Hv, Hf = O.obs_blocks(np.asarray(x, dtype=np.float64), idf)
    H = np.zeros((2 * len(idf), len(x)))
    for i, j in enumerate(idf):
        f = 3 + 2 * (j - 1)
        H[2 * i:2 * i + 2, 0:3] = Hv[i]
        H[2 * i:2 * i + 2, f:f + 2] = Hf[i]
    return H


# ---- the accumulator rules ---------------------------------------------------------------------------------------------------------
def acc_predict(phi, p, v, g, dt):
    """phi[0:3, :] <- Gv phi[0:3, :] with the local heading p before the step."""
    Gv = np.array([[1.0, 0.0, -v * dt * math.sin(g + p)], [0.0, 1.0, v * dt * math.cos(g + p)], [0.0, 0.0, 1.0]])
    out = np.array(phi)
    out[0:3] = Gv @ phi[0:3]
    return out


def acc_augment(phi, p, zn):
    """phi gains the rows Gxv phi[0:3, :] of every new observation (r, b) at the local heading p."""
    zn = np.asarray(zn, dtype=np.float64).reshape(2, -1)
    rows = [phi]
    for i in range(zn.shape[1]):
        r, b = zn[0, i], zn[1, i]
        Gxv = np.array([[1.0, 0.0, -r * math.sin(p + b)], [0.0, 1.0, r * math.cos(p + b)]])
        rows.append(Gxv @ phi[0:3])
    return np.vstack(rows)


def update_parts(x, P, z, idf, R):
    """(H, C, W, g, v, S) of the Cholesky-form update at the local state (x, P): C = inv(chol(S))' upper, W = P H' C, g = C C' v."""
    v, PHt, S = O._update_front(x, P, z, R, idf)
    Uc = np.linalg.cholesky(S).T
    C = np.linalg.inv(Uc)
    return dense_H(x, idf), C, PHt @ C, C @ (C.T @ v), v, S


def acc_update(phi, psi, theta, x, P, z, idf, R, dtype=np.float64):
    """theta += E' g, psi += Y' Y, phi -= W Y with E = H phi, Y = C' E and W rounded once to the state's dtype."""
    H, C, W, g, _v, _S = update_parts(x, P, z, idf, R)
    W = W.astype(dtype).astype(np.float64)
    E = H[:, :phi.shape[0]] @ phi
    Y = C.T @ E
    return phi - W @ Y, psi + Y.T @ Y, theta + E.T @ g


# ---- close -------------------------------------------------------------------------------------------------------------------------
def local_to_global(ids, n_old, n_a):
    """Global state index of every local one: the vehicle, ids, then the landmarks added locally (appended behind n_old)."""
    sel = select_indices(ids)
    return np.concatenate([sel, n_old + np.arange(n_a - len(sel), dtype=np.int64)])


def close(xg, Pg, ids, x_a, P_a, phi, psi, theta):
    """The five steps of close on dense arrays; returns the new global (x, P)."""
    xg, Pg = np.asarray(xg, dtype=np.float64), np.asarray(Pg, dtype=np.float64)
    n_old, n_a = len(xg), len(x_a)
    sel = select_indices(ids)
    l2g = local_to_global(ids, n_old, n_a)
    n_new = n_old + n_a - len(sel)
    B = np.setdiff1d(np.arange(n_old), sel)
    A0 = Pg[np.ix_(B, sel)]                                               # P_ba at open
    x = np.zeros(n_new)
    P = np.zeros((n_new, n_new))
    x[:n_old] = xg
    P[:n_old, :n_old] = Pg
    x[B] = xg[B] + A0 @ theta                                             # 1
    P[np.ix_(B, B)] = Pg[np.ix_(B, B)] - (A0 @ psi) @ A0.T                # 2
    Pab = phi @ A0.T                                                      # 3
    P[np.ix_(l2g, B)] = Pab
    P[np.ix_(B, l2g)] = Pab.T
    x[l2g] = x_a                                                          # 4
    P[np.ix_(l2g, l2g)] = P_a
    return x, P


def gamma(k, w):
    return k * w / (1.0 - k * w)


def close_bound(xg, Pg, ids, n_a, phi, psi, theta, x_new, P_new, dtype):
    """The header's per-entry bound of close against the exact five steps on the same inputs: (Bx, BP), zero on x_a and P_aa
    (exact copies)."""
    u = U[np.dtype(dtype)]
    xg, Pg = np.asarray(xg, dtype=np.float64), np.asarray(Pg, dtype=np.float64)
    n_old = len(xg)
    sel = select_indices(ids)
    n0 = len(sel)
    K = (n0 + 15) // 16 * 16
    l2g = local_to_global(ids, n_old, n_a)
    B = np.setdiff1d(np.arange(n_old), sel)
    A0 = np.abs(Pg[np.ix_(B, sel)])
    Bx = np.zeros(len(x_new))
    BP = np.zeros(P_new.shape)
    Bx[B] = u * np.abs(x_new[B]) + gamma(n0 + 1, V) * (np.abs(xg[B]) + A0 @ np.abs(theta))
    Tabs = np.abs(Pg[np.ix_(B, sel)] @ psi)
    chain = gamma(n0, V) * (A0 @ np.abs(psi))                             # the double chain behind every T_rk
    That = Tabs * (1 + u) + chain                                         # |T| as computed
    BP[np.ix_(B, B)] = (u * np.abs(P_new[np.ix_(B, B)]) + (gamma(K + 1, u) + u) * (That @ A0.T) + (1 + u) * (chain @ A0.T))
    ab = u * np.abs(P_new[np.ix_(l2g, B)]) + gamma(n0, V) * (np.abs(phi) @ A0.T)
    BP[np.ix_(l2g, B)] = ab
    BP[np.ix_(B, l2g)] = ab.T
    return Bx, BP


# ---- the whole filter --------------------------------------------------------------------------------------------------------------
class LocalRef:
    """open at construction; predict / update / augment on the local state with the oracle's sparse forms; close() returns the
    new global (x, P).  ``dtype``: the state's dtype, i.e. what W is rounded to."""

    def __init__(self, xg, Pg, ids, dtype=np.float64):
        self.xg, self.Pg = np.array(xg, dtype=np.float64), np.array(Pg, dtype=np.float64)
        self.ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        self.dtype = dtype
        s = select_indices(self.ids)
        self.x, self.P = self.xg[s].copy(), self.Pg[np.ix_(s, s)].copy()
        self.n0 = len(s)
        self.phi, self.psi, self.theta = np.eye(self.n0), np.zeros((self.n0, self.n0)), np.zeros(self.n0)

    def predict(self, v, g, w, Q, dt):
        self.phi = acc_predict(self.phi, self.x[2], v, g, dt)
        self.x, self.P = O.predict_sparse(self.x, self.P, v, g, w, np.asarray(Q, float), dt)

    def update(self, z, idf, R):
        self.phi, self.psi, self.theta = acc_update(self.phi, self.psi, self.theta, self.x, self.P, z, idf, R, self.dtype)
        self.x, self.P = O.update_sparse(self.x, self.P, z, np.asarray(R, float), idf)

    def augment(self, zn, R):
        self.phi = acc_augment(self.phi, self.x[2], zn)
        self.x, self.P = O.add_features_sparse(self.x, self.P, zn, np.asarray(R, float))

    def close(self):
        return close(self.xg, self.Pg, self.ids, self.x, self.P, self.phi, self.psi, self.theta)


# ---- the call surface sim(..., local_radius=r) drives, over the oracle: what the GPU run is compared with ------------------------
class _Pose:
    def __init__(self, area):
        self._area = area

    def pose(self):
        return self._area.ref.x[0:3].copy()


class RefArea:
    """LocalArea's surface over LocalRef."""

    def __init__(self, parent, ids):
        self.parent = parent
        self.ids = np.asarray(ids, dtype=np.int32).reshape(-1)
        self.ref = LocalRef(parent.x, parent.cov, self.ids)
        self.N_open = parent.N
        self.state = _Pose(self)
        self.steps = 0

    def info(self):
        n_a = len(self.ref.x)
        return {"open": 1, "n0": self.ref.n0, "n_a": n_a, "added": (n_a - self.ref.n0) // 2, "steps": self.steps, "N_open": self.N_open}

    def global_ids(self):
        return np.concatenate([self.ids, self.N_open + 1 + np.arange(self.info()["added"], dtype=np.int32)]).astype(np.int32)

    def predict(self, v, g, w, Q, dt):
        self.ref.predict(v, g, w, Q, dt)

    def associate(self, z, R, gate1, gate2):
        return O.associate_sparse(self.ref.x, self.ref.P, z, np.asarray(R, float), gate1, gate2)

    def update(self, zf, R, idf):
        if np.asarray(zf).size:
            self.ref.update(zf, np.asarray(idf).reshape(-1), R)

    def add_features(self, zn, R):
        if np.asarray(zn).size:
            self.ref.augment(zn, R)

    def close(self):
        self.parent.x, self.parent.cov = self.ref.close()
        return self.N_open + 1

    def destroy(self):
        pass


class RefFilter(O.OracleEKF):
    """The oracle's filter object plus the two calls sim(..., local_radius=r) makes on the global state."""

    def __init__(self, x, P):
        super().__init__(x, P, sparse=True)

    @property
    def N(self):
        return (len(self.x) - 3) // 2

    def landmarks_within(self, cx, cy, r):
        lm = self.x[3:].reshape(-1, 2)
        return (np.flatnonzero(np.hypot(lm[:, 0] - cx, lm[:, 1] - cy) <= r) + 1).astype(np.int32)

    def local(self, ids):
        return RefArea(self, ids)
