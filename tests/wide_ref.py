"""Dense fp64 NumPy restatement of the rule of include/ext/slamhip_wide.h: the JOINT update of up to 64 range-bearing observations,
the residuals at x, the Jacobians at the linearisation points (lin, first) of a first-estimates filter (tests/fej_ref.py) -- or at x
itself, which is then the oracle's Cholesky-form update.  tests/fej_ref.update is the same rule and asserts m <= 8; this one takes
any m <= 64 and is built on the same pieces (fej_ref.dense_H, linear_ref.chol_lower).

Also here: the scenes of tests/test_wide_ref_cpu.py and tests/test_gpu_ekf_wide.py -- tests/iterated_ref.py's designed base state,
hardened around a seeded permutation of landmark ids that starts with the landmark straddling a tile edge and the last landmark --
and the displaced linearisation points of tests/test_gpu_ekf_fej.py."""
import numpy as np

from oracle import ekf_ref as O
from tests import fej_ref as F
from tests import iterated_ref as IR
from tests.linear_ref import chol_lower

MAXOBS = 64
# (N, m, the last id repeats the first): k_p = 32 / 64 / 96 / 128 rows of S and 16 .. 128 panel columns; n = 143 and 403
SCENES = [(70, 1, False), (70, 9, False), (70, 17, False), (70, 33, True), (70, 64, False), (200, 48, False), (200, 64, False),
          (200, 64, True)]
SEEDS = (3, 5)


def update(x, P, lin, first, z, R, idf):
    """The residuals at x, the Jacobian at (lin, first), then the reference's Cholesky form on all m observations at once.  Returns
    (x, P, out[4], H); x and P come back unchanged (copies) after a failing pivot (out[3] >= 0)."""
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
        H = F.dense_H(lin, first, idf, len(x))
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


def update_at_estimates(x, P, z, R, idf):
    """The points re-set to x: the standard filter's update (f == NULL of the library)."""
    lin, first = F.create(x)
    return update(x, P, lin, first, z, R, idf)


def update_batches(x, P, lin, first, z, R, idf):
    """More than 64 observations: consecutive batches of 64.  Returns (x, P, [out of every batch])."""
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    idf = np.asarray(idf).reshape(-1)
    outs = []
    for s in range(0, z.shape[1], MAXOBS):
        x, P, out, _ = update(x, P, lin, first, z[:, s:s + MAXOBS], R, idf[s:s + MAXOBS])
        outs.append(out)
    return x, P, outs


def scene_ids(N, m, dtype, seed, repeat=False):
    """A seeded permutation of 1 .. N whose first entry is the straddler and whose second is N, cut to m; optionally the last id
    repeats the first (that landmark is observed twice)."""
    s = IR.STRADDLER[dtype]
    rest = [j for j in np.random.default_rng(500 + seed).permutation(N) + 1 if j not in (s, N)]
    ids = np.array(([s, N] + rest)[:m], dtype=np.int64)
    if repeat:
        ids[-1] = ids[0]
    return ids


def scene(N, m, dtype, seed, repeat=False):
    """(x, P, z, ids): x and P hold values of the dtype exactly, so an upload changes nothing."""
    ids = scene_ids(N, m, dtype, seed, repeat)
    x, P = IR.base_state(N, dtype)
    x, P, z = IR.harden(x, P, ids, seed)
    t = IR.NP_DTYPE[dtype]
    return x.astype(t).astype(np.float64), P.astype(t).astype(np.float64), z, ids


def displaced(x, seed):
    """The linearisation points of the tests (tests/test_gpu_ekf_fej.py::displaced): the estimates moved by (0.3, -0.2, 0.05) and
    N(0, 0.2^2) per landmark coordinate."""
    rng = np.random.default_rng(seed)
    return x[0:3] + [0.3, -0.2, 0.05], x[3:] + rng.normal(0.0, 0.2, len(x) - 3)
