"""One table of the calls that change the map, each with a DESIGNED scene: a state before the call, the call, and observations
for the gating afterwards -- chosen so that the side state the gating keeps beside x and P (tests/gate_cache_ref.py) would take
another decision than the exact gate if the call had left it as it was.  tests/test_gate_cache_cpu.py shows that property from
the fp64 references alone; tests/test_gpu_ekf_gate_cache.py makes the calls on primed handles.  Host-only: a scene's `call` is
the only part that touches the device.

The recipe (N = 70: two tile rows in fp32, three in fp64; landmark 63 straddles a tile edge in both):
  * P_vv about 1e-6, every landmark variance about 1e-4, R = diag(0.01, 1e-4): rho is about 0.5 m under that bound;
  * (a)(b): a landmark comes out of the call with variance 4 m^2 and is observed 3 m off radially (nis about 2.2, inside gate1;
    3 m is six times the old rho, and v_0^2 = 9 is 35 times gate2 B_0 of the old bound);
  * (c): a landmark is moved by more than twice the rho of the bound the device holds afterwards -- a loose landmark (variance 4,
    rho about 14 m) by an update with a given id and a 34 m innovation (an update with known ids applies no gate) -- or the call
    renumbers the map, so that the item of the observed landmark's index carries another landmark's mean.
Condition (r) is the other direction: a call after which the largest variance is far BELOW the bound held before has to make the
device recompute it (the Joseph-form update); a stale bound is then still valid and changes no decision, so the observable is the
number of landmarks the grid query evaluates (tests/gate_cache_ref.evaluated_bounds): at least twice as many under the old bound.
`sensitive` names the conditions of tests/gate_cache_ref.stale_would_miss a row's targets satisfy with a factor of 2, or is
"control" (`why` then says why the call cannot invalidate anything, or why it cannot be made sensitive)."""
import math

import numpy as np

from oracle import ekf_ref as O
from tests import copy_ref as CR
from tests import fej_ref as FR
from tests import handover_ref as HR
from tests import iterated_ref as IR
from tests import join_ref as JR
from tests import linear_ref as LR
from tests import merge_ref as MR
from tests import transform_ref as X
from tests import wide_ref as WR
from tests.gate_cache_ref import f

N = 70
CAP = 80                                    # landmark capacity of every handle
GATE1, GATE2 = 4.0, 25.0
R = np.diag([0.01, 1e-4])
R_LOOSE = np.diag([4.0, 1e-4])              # add_features with this R: the new landmark's radial variance is 4
Q = np.diag([0.25, (3 * math.pi / 180) ** 2])
POSE = np.array([50.0, 50.0, 0.3])
T = 63                                      # the designed landmark: rows 127 | 128, on either side of a tile edge in both dtypes
MATCH = [5, 20, 31, 44, 70]                 # tight landmarks observed beside it (31 straddles the first fp64 tile edge)
MOVE = 34.0                                 # metres: more than twice rho = 14.16 of a bound of 4
OFF = 3.0                                   # metres off radially: nis = 9 / 4.01 under a variance of 4
NEW = np.array([150.0, 2.0])                # an observation far from every landmark: a new feature
WIDE1, WIDE2 = 400.0, 1000.0                # the gates of an observe() that has to ACCEPT a 34 m innovation (nis about 290)


class Scene:
    """before: (x, P) uploaded and primed; call(pkg, st, mode): the call under test on a primed handle (mode: the handle's gate
    mode) -- returns None, or {"query": state, "close": fn} when the gating to check is that of another handle; after: the
    expected (x, P) from the fp64 references; z: the observations [2, nz]; targets: (observation index, landmark id, conditions);
    x_old: the means a stale grid item would carry (default: before's); stale_bound: for condition (r), the bound the device
    would still hold if the call had not made it recompute."""

    def __init__(self, before, call, after, z, targets=(), x_old=None, stale_bound=None):
        self.stale_bound = stale_bound
        self.before = (np.asarray(before[0], dtype=np.float64), np.asarray(before[1], dtype=np.float64))
        self.call = call
        self.after = (np.asarray(after[0], dtype=np.float64), np.asarray(after[1], dtype=np.float64))
        self.z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        self.targets = tuple(targets)
        self.x_old = self.before[0] if x_old is None else np.asarray(x_old, dtype=np.float64)


class Row:
    def __init__(self, name, lib, entries, sensitive, build, rebuild=None, recomputed=False, why="", tail=None):
        assert sensitive == "control" or set(sensitive) <= set("abcr")
        assert sensitive != "control" or why
        self.name, self.lib, self.entries, self.sensitive = name, lib, tuple(entries), sensitive
        self.build = build                  # build(dtype) -> Scene
        self.rebuild = rebuild              # the grid handle's next query: "forced" = exactly one rebuild, "kept" = none, None = not checked
        self.recomputed = recomputed        # the call makes the device recompute its variance bound (else it keeps or raises it)
        self.why = why
        self.tail = tail                    # landmarks the grid handle's next query reads from the tail (in_grid stays N); None = not checked


# ---- the base state ---------------------------------------------------------------------------------------------------------------
def _means():
    rng = np.random.default_rng(7001)
    xy = np.array([(2.0 + 12.0 * i, 8.0 + 12.0 * k) for k in range(8) for i in range(9)][:N])
    return xy + rng.uniform(-1.0, 1.0, xy.shape)


def base(var=None, at=None, n_lm=N):
    """(x, P): the pose, n_lm landmarks on a jittered 12 m lattice, P = diag + a rank-3 term (every pair is correlated).  var:
    {landmark: variance}, default 1e-4; at: {landmark: (x, y)}."""
    var, at = dict(var or {}), dict(at or {})
    lm = _means()[:n_lm]
    for j, p in at.items():
        lm[j - 1] = p
    n = 3 + 2 * n_lm
    d = np.full(n, 1e-4)
    d[0:3] = [1e-6, 1e-6, 1e-8]
    for j, v in var.items():
        d[f(j):f(j) + 2] = v
    A = np.random.default_rng(7002).normal(0.0, 3e-4, (3 + 2 * N, 3))[:n]
    A[2] *= 0.1
    P = np.diag(d) + A @ A.T
    return np.concatenate([POSE, lm.reshape(-1)]), (P + P.T) / 2


def radial(x, j, d):
    """The mean of landmark j displaced by d metres along the ray from the pose."""
    p = x[f(j):f(j) + 2] - x[0:2]
    return x[f(j):f(j) + 2] + d * p / np.linalg.norm(p)


def obs(x, j, dr=0.0, db=0.0):
    zp, _ = O.predict_observation(x, j)
    return np.asarray(zp, dtype=np.float64).reshape(2) + [dr, db]


def observations(x, matches, targets):
    """z and the target list: the tight landmarks `matches` (2 cm, 2 mrad off), then the targets (landmark, metres off radially,
    conditions), then the new feature."""
    cols = [obs(x, j, 0.02, 0.002) for j in matches]
    tl = []
    for j, off, conds in targets:
        tl.append((len(cols), j, conds))
        cols.append(obs(x, j, off))
    cols.append(NEW)
    return np.stack(cols, axis=1), tl


def _loose_after(move=MOVE):
    """before: all tight; after: landmark T 34 m further out with variance 4 -- the pair of the calls that replace the state."""
    x0, P0 = base()
    x1, P1 = base(var={T: 4.0}, at={T: radial(x0, T, move)})
    return (x0, P0), (x1, P1)


# ---- product library ----------------------------------------------------------------------------------------------------------------
def _replaced(how):
    def build(dtype):
        before, after = _loose_after()
        z, tl = observations(after[0], MATCH, [(T, OFF, "abc")])
        return Scene(before, lambda pkg, st, mode: how(pkg, st, after, dtype), after, z, tl)
    return build


def _set_state(pkg, st, after, dtype):
    st.set_state(*after)


def _set_state_device(pkg, st, after, dtype):
    import torch
    tdt = torch.float32 if dtype == "f32" else torch.float64
    xd = torch.as_tensor(after[0], dtype=tdt, device="cuda")
    Pd = torch.as_tensor(after[1], dtype=tdt, device="cuda").contiguous()      # symmetric: row-major == column-major
    torch.cuda.synchronize()
    st.set_state_device(xd.data_ptr(), Pd.data_ptr(), len(after[0]), len(after[0]))
    st.sync()


def _raw_write(pkg, st, after, dtype):
    """Landmark T's mean and its two variances written through the raw device views, then slam_ekf_state_written."""
    import torch
    from tests import strip_ref as SR
    view, ld, E = SR.raw_view(st)
    d_x = st.device_ptrs()[0]

    class _X:
        __cuda_array_interface__ = {"shape": (st.n,), "typestr": "<f4" if dtype == "f32" else "<f8", "data": (d_x, False), "version": 2}
    xv = torch.as_tensor(_X(), device="cuda")
    L = E.bit_length() - 1
    rows = np.array([f(T), f(T) + 1])
    xv[torch.as_tensor(rows, device="cuda")] = torch.as_tensor(after[0][rows], dtype=xv.dtype, device="cuda")
    view[torch.as_tensor(SR.p_off(ld, L, rows, rows), device="cuda")] = 4.0
    torch.cuda.synchronize()
    st.state_written()


def _raw_build(dtype):
    x0, P0 = base()
    x1, P1 = x0.copy(), P0.copy()
    x1[f(T):f(T) + 2] = radial(x0, T, MOVE)
    P1[f(T), f(T)] = P1[f(T) + 1, f(T) + 1] = 4.0                            # the correlations stay as they were
    z, tl = observations(x1, MATCH, [(T, OFF, "abc")])
    return Scene((x0, P0), lambda pkg, st, mode: _raw_write(pkg, st, (x1, P1), dtype), (x1, P1), z, tl)


def _moved(apply_ref, do, var=4.0, wide=False):
    """A loose landmark T moved 34 m by an update with a given id.  apply_ref(x, P, z, ids) -> (x, P); do(pkg, st, z, ids)."""
    def build(dtype):
        x0, P0 = base(var={T: var})
        gain = var / (var + R[0, 0])
        zu = obs(x0, T, MOVE / gain).reshape(2, 1)
        x1, P1 = apply_ref(x0, P0, zu, [T])
        z, tl = observations(x1, MATCH, [(T, 0.05, "c")])
        return Scene((x0, P0), lambda pkg, st, mode: do(pkg, st, zu, [T]), (x1, P1), z, tl)
    return build


def _update(form="cholesky", use_async=False):
    def do(pkg, st, z, ids):
        if use_async:
            st.set_async(True)
        st.update(z, R, ids, form=form)
        if use_async:
            st.sync()
            st.set_async(False)
    return do


NEAR = 41                                   # six metres from the vehicle: its lateral variance after an update is tiny as well


def _joseph_bound_build(dtype):
    """Landmark 41 (variance 4, the bound) is observed a centimetre off and updated in the Joseph form: afterwards every variance is
    at most about 0.01, and the grid query's reach has to be that of the recomputed bound (under a metre), not 14 m."""
    x0, P0 = base(var={NEAR: 4.0})
    zu = obs(x0, NEAR, 0.01).reshape(2, 1)
    x1, P1 = O.update_joseph_sparse(x0, P0, zu, R, np.array([NEAR]))
    z, tl = observations(x1, [32, 40, NEAR, 42], [])
    return Scene((x0, P0), lambda pkg, st, mode: st.update(zu, R, [NEAR], form="joseph"), (x1, P1), z, tl, stale_bound=4.0)


def _many_updates(count):
    """`count` updates between two queries: the first moves T, the others touch tight landmarks by a centimetre."""
    def build(dtype):
        x, P = base(var={T: 4.0})
        x0, P0 = x, P
        steps = []
        for u in range(count):
            j = T if u == 0 else 1 + (7 * u) % 60
            zu = obs(x, j, MOVE * (4.01 / 4.0) if u == 0 else 0.01).reshape(2, 1)
            steps.append((zu, [j]))
            x, P = O.update_sparse(x, P, zu, R, np.array([j]))
        z, tl = observations(x, MATCH, [(T, 0.05, "c")])

        def call(pkg, st, mode):
            for zu, ids in steps:
                st.update(zu, R, ids)
        return Scene((x0, P0), call, (x, P), z, tl)
    return build


ZN = np.array([[75.0, 70.0], [2.2, -2.0]])                                 # two new features beyond the lattice


def _appended(apply_ref, do, bound_invalid=False):
    def build(dtype):
        x0, P0 = base()
        xa, Pa = x0, P0
        zj = obs(x0, 12, 0.01).reshape(2, 1)
        if bound_invalid:
            xa, Pa = O.update_joseph_sparse(x0, P0, zj, R, np.array([12]))
        x1, P1 = apply_ref(xa, Pa, ZN, R_LOOSE)
        z, tl = observations(x1, MATCH, [(N + 1, OFF, "ab")])

        def call(pkg, st, mode):
            if bound_invalid:
                st.update(zj, R, [12], form="joseph")                        # pmax_valid = 0 and no query before the augment
            do(pkg, st, ZN, R_LOOSE)
        return Scene((x0, P0), call, (x1, P1), z, tl)
    return build


def _wide_observations(x0, P0):
    """What the observe() rows pass: T 34 m out, landmark 12 a centimetre off, one new feature -- decided so under the wide gates."""
    zo = np.stack([obs(x0, T, MOVE * 4.01 / 4.0), obs(x0, 12, 0.01), np.array([75.0, 2.2])], axis=1)
    nis, nd = O.association_table_sparse(x0, P0, zo, R)
    assert O.assoc_vector(nis, nd, WIDE1, WIDE2).tolist() == [T, 12, -1]
    assert min(abs(nis[0, T - 1] - WIDE1) / WIDE1, abs(nis[2].min() - WIDE2) / WIDE2) > 0.1
    return zo


def _observe_build(dtype):
    """observe() with gates wide enough to accept the 34 m innovation of the loose landmark: matched -> update, new -> appended."""
    x0, P0 = base(var={T: 4.0})
    zo = _wide_observations(x0, P0)
    x1, P1 = O.update_sparse(x0, P0, zo[:, :2], R, np.array([T, 12]))
    x1, P1 = O.add_features_sparse(x1, P1, zo[:, 2:], R)
    z, tl = observations(x1, MATCH, [(T, 0.05, "c")])

    def call(pkg, st, mode):
        a = st.observe(zo, R, WIDE1, WIDE2)
        assert a.tolist() == [T, 12, -1], a
    return Scene((x0, P0), call, (x1, P1), z, tl)


GONE = [10, 40]


def _remove_build(dtype):
    x0, P0 = base()
    keep = np.delete(np.arange(len(x0)), [i for j in GONE for i in (f(j), f(j) + 1)])
    x1, P1 = x0[keep], P0[np.ix_(keep, keep)]
    m = [5, 19, 30, 42, 68]                                                  # old 5, 20, 31, 44, 70
    z, tl = observations(x1, m[:1], [(j, 0.02, "c") for j in m[1:] + [T - 2]])
    return Scene((x0, P0), lambda pkg, st, mode: st.remove_landmarks(GONE), (x1, P1), z, tl)


def _merge_build(dtype):
    """Landmark 40 is landmark 12 entered twice (5 mm apart): merged exactly, 40 leaves, everything behind it is renumbered."""
    x0, P0 = base(at={40: _means()[11] + [0.004, -0.003]})
    x1, P1, _ni = MR.merge(x0, P0, [(12, 40)])
    z, tl = observations(x1, [5, 12, 20], [(j, 0.02, "c") for j in (43, 69, T - 1)])
    return Scene((x0, P0), lambda pkg, st, mode: st.merge_landmarks([(12, 40)]), (x1, P1), z, tl)


def _control(apply_ref, do):
    def build(dtype):
        x0, P0 = base()
        x1, P1 = apply_ref(x0, P0)
        z, tl = observations(x1, MATCH + [T], [])
        return Scene((x0, P0), lambda pkg, st, mode: do(pkg, st), (x1, P1), z, tl)
    return build


# ---- frame --------------------------------------------------------------------------------------------------------------------------
G_ALIGN = (1000.0, -2000.0, -2.9)
ALIGN_IDS = [2, 9, 17, 26, 35]


def _align_build(dtype):
    x0, P0 = base()
    x1, P1 = X.transform(x0, P0, *G_ALIGN)
    surveyed = np.stack([x1[[f(j) for j in ALIGN_IDS]], x1[[f(j) + 1 for j in ALIGN_IDS]]])
    z, tl = observations(x1, [], [(j, 0.02, "c") for j in MATCH + [T]])
    return Scene((x0, P0), lambda pkg, st, mode: st.align(ALIGN_IDS, surveyed), (x1, P1), z, tl)


# ---- join ---------------------------------------------------------------------------------------------------------------------------
def _join_build(merge):
    def build(dtype):
        x0, P0 = base()
        pb = np.array([1.0, 0.5, 0.05])
        lmB = [np.array([70.0, 10.0]), np.array([-60.0, 30.0])]
        varB = [4.0, 4.0]
        if merge:                                                            # B's first landmark IS landmark 20, seen from B's pose
            c, s = math.cos(POSE[2]), math.sin(POSE[2])
            Rw = np.array([[c, -s], [s, c]])
            lmB[0] = Rw.T @ (x0[f(20):f(20) + 2] + [0.004, 0.003] - POSE[0:2])
            varB[0] = 1e-4
        xB = np.concatenate([pb, lmB[0], lmB[1]])
        PB = np.diag([1e-6, 1e-6, 1e-8, varB[0], varB[0], varB[1], varB[1]])
        x1, P1 = (np.asarray(a, dtype=np.float64) for a in JR.join(x0, P0, xB, PB))
        target = N + 2
        if merge:
            x1, P1, _ni = MR.merge(x1, P1, [(20, N + 1)])
            target = N + 1
        z, tl = observations(x1, MATCH, [(target, OFF, "ab")])

        def call(pkg, st, mode):
            sub = st.submap(8)
            try:
                sub.set_state(xB, PB)
                if merge:
                    first, ni = st.join(sub, merge_gate=9.0)
                    assert first == N + 1 and ni[N] == 20 and ni[N + 1] == N + 1, (first, ni[N:])
                else:
                    assert st.join(sub) == N + 1
            finally:
                sub.close()
        return Scene((x0, P0), call, (x1, P1), z, tl)
    return build


# ---- copy ---------------------------------------------------------------------------------------------------------------------------
SELECT_IDS = [2, 1] + [j for j in range(3, N + 1) if j not in GONE]


def _from_other(select):
    def build(dtype):
        before, src = _loose_after()
        after, target = src, T
        if select:
            s = CR.index_map(N, SELECT_IDS)
            after, target = (src[0][s], src[1][np.ix_(s, s)]), T - 2
        matches = [SELECT_IDS.index(j) + 1 for j in MATCH] if select else MATCH
        z, tl = observations(after[0], matches, [(target, OFF, "abc")])

        def call(pkg, st, mode):
            other = pkg.EKFSlamState(src[0], src[1], dtype=dtype, max_landmarks=CAP)
            try:
                if select:
                    st.select_from(other, SELECT_IDS)
                else:
                    st.copy_from(other)
                st.sync()
            finally:
                other.close()
        return Scene(before, call, after, z, tl)
    return build


# ---- handover -------------------------------------------------------------------------------------------------------------------------
PARTICLES = 64


def _handover_build(dtype):
    """64 designed particles around the `after` state of _loose_after: poses spread by a millimetre, every landmark's mean by a
    centimetre with a within-particle variance of 1e-6 -- 4.0 for landmark T.  The joint Gaussian is tests/handover_ref's."""
    before, want = _loose_after()
    rng = np.random.default_rng(7003)
    npdt = HR.NP_DTYPE[dtype]
    pose = (want[0][0:3, None] + rng.normal(0.0, 1.0, (3, PARTICLES)) * np.array([[1e-3], [1e-3], [1e-4]])).astype(npdt)
    logw = rng.normal(0.0, 0.1, PARTICLES).astype(npdt)
    lm = np.zeros((N, 5, PARTICLES))
    lm[:, 0:2] = want[0][3:].reshape(N, 2, 1) + rng.normal(0.0, 1e-2, (N, 2, PARTICLES))
    lm[:, 2] = lm[:, 4] = 1e-6
    lm[T - 1, 2] = lm[T - 1, 4] = 4.0
    lm = lm.astype(npdt)
    ref = HR.pf_to_ekf(pose, logw, lm, np.arange(1, N + 1), dtype)
    after = (ref["x"], ref["P"])
    z, tl = observations(after[0], MATCH, [(T, OFF, "abc")])

    def call(pkg, st, mode):
        sh = pkg.PFShard(PARTICLES, N, 11, dtype=dtype)
        try:
            sh.upload(pose, logw, lm, np.ones(N))
            sh.to_ekf_into(st, None)
        finally:
            sh.close()
    return Scene(before, call, after, z, tl)


# ---- linear ---------------------------------------------------------------------------------------------------------------------------
def _fix_landmark_build(dtype):
    x0, P0 = base(var={T: 4.0})
    fix = radial(x0, T, MOVE * 4.01 / 4.0)
    H = LR.dense_H(len(x0), [{f(T): 1.0}, {f(T) + 1: 1.0}])
    x1, P1, _out = LR.update(x0, P0, H, fix, 0.01 * np.eye(2))
    z, tl = observations(x1, MATCH, [(T, 0.05, "c")])
    return Scene((x0, P0), lambda pkg, st, mode: st.fix_landmark(T, fix, 0.01 * np.eye(2)), (x1, P1), z, tl)


def _constrain_build(dtype):
    """Landmark T (loose) lies `dxy` from landmark 62 (tight): it moves there."""
    x0, P0 = base(var={T: 4.0})
    dxy = radial(x0, T, MOVE * 4.01 / 4.0) - x0[f(62):f(62) + 2]
    H = LR.dense_H(len(x0), [{f(T): 1.0, f(62): -1.0}, {f(T) + 1: 1.0, f(62) + 1: -1.0}])
    x1, P1, _out = LR.update(x0, P0, H, dxy, 0.01 * np.eye(2))
    z, tl = observations(x1, MATCH, [(T, 0.05, "c")])
    return Scene((x0, P0), lambda pkg, st, mode: st.constrain_landmarks(62, T, dxy, 0.01 * np.eye(2)), (x1, P1), z, tl)


XV = POSE + [0.3, -0.2, 0.02]
GV = np.array([[1.0, 0.0, -0.2], [0.0, 1.0, 0.3], [0.0, 0.0, 1.0]])
QV = np.diag([1e-6, 1e-6, 1e-8])
ODO = np.array([0.3, -0.1, 0.02])


# ---- iterated, fej, wide ----------------------------------------------------------------------------------------------------------------
def _fej_ref(fn):
    def apply_ref(x, P, z, ids):
        lin, first = FR.create(x)
        return fn(x, P, lin, first, z, R, np.asarray(ids))[0:2]
    return apply_ref


def _with_fej(method):
    def do(pkg, st, z, ids):
        obj = st.fej()
        try:
            getattr(obj, method)(z, R, ids)
        finally:
            obj.close()
    return do


def _fej_add(pkg, st, zn, Rn):
    obj = st.fej()
    try:
        obj.add_features(zn, Rn)
    finally:
        obj.close()


def _fej_add_ref(x, P, zn, Rn):
    lin, first = FR.create(x)
    return FR.add_features(x, P, lin, first, zn, Rn)[0:2]


def _fej_predict(pkg, st):
    obj = st.fej()
    try:
        obj.predict(2.0, 0.05, 4.0, Q, 0.025)
    finally:
        obj.close()


def _fej_predict_ref(x, P):
    lin, first = FR.create(x)
    return FR.predict(x, P, lin, first, 2.0, 0.05, 4.0, Q, 0.025)[0:2]


def _fej_observe_build(dtype):
    x0, P0 = base(var={T: 4.0})
    zo = _wide_observations(x0, P0)
    lin, first = FR.create(x0)
    x1, P1 = FR.update(x0, P0, lin, first, zo[:, :2], R, np.array([T, 12]))[0:2]
    x1, P1 = FR.add_features(x1, P1, lin, first, zo[:, 2:], R)[0:2]
    z, tl = observations(x1, MATCH, [(T, 0.05, "c")])

    def call(pkg, st, mode):
        obj = st.fej()
        try:
            a = obj.observe(zo, R, WIDE1, WIDE2)
            assert a.tolist() == [T, 12, -1], a
        finally:
            obj.close()
    return Scene((x0, P0), call, (x1, P1), z, tl)


def _observe_iterated_build(dtype):
    x0, P0 = base(var={T: 4.0})
    zo = _wide_observations(x0, P0)
    x1, P1, _out = IR.update(x0, P0, zo[:, :2], R, np.array([T, 12]))
    x1, P1 = O.add_features_sparse(x1, P1, zo[:, 2:], R)
    z, tl = observations(x1, MATCH, [(T, 0.05, "c")])

    def call(pkg, st, mode):
        a, _res = st.observe_iterated(zo, R, WIDE1, WIDE2)
        assert a.tolist() == [T, 12, -1], a
    return Scene((x0, P0), call, (x1, P1), z, tl)


# ---- local ----------------------------------------------------------------------------------------------------------------------------
AREA = [61, 62, T, 64]
VAR_LOCAL = 0.04                            # the moved landmark of the close row: the OLD bound has to stay well below 4


def _local_steps(x0, var):
    gain = var / (var + R[0, 0])
    return obs(x0, T, MOVE / gain).reshape(2, 1), np.array([[75.0], [2.2]])


def _local_close_build(dtype):
    """An area over four landmarks: T (variance 0.04) moved 34 m, one landmark appended with a radial variance of 4.  The expected
    state is the full filter's on the global state, which the compressed filter equals up to rounding (tests/local_ref.py)."""
    x0, P0 = base(var={T: VAR_LOCAL})
    zu, zn = _local_steps(x0, VAR_LOCAL)
    x1, P1 = O.update_sparse(x0, P0, zu, R, np.array([T]))
    x1, P1 = O.add_features_sparse(x1, P1, zn, R_LOOSE)
    z, tl = observations(x1, MATCH, [(T, 0.05, "c"), (N + 1, 3.5, "ab")])

    def call(pkg, st, mode):
        area = st.local(AREA)
        try:
            area.update(zu, R, [AREA.index(T) + 1])
            area.add_features(zn, R_LOOSE)
            assert area.close() == N + 1
        finally:
            area.destroy()
    return Scene((x0, P0), call, (x1, P1), z, tl)


def _local_abort_build(dtype):
    x0, P0 = base(var={T: VAR_LOCAL})
    zu, zn = _local_steps(x0, VAR_LOCAL)
    z, tl = observations(x0, MATCH + [T], [])

    def call(pkg, st, mode):
        area = st.local(AREA)
        try:
            area.update(zu, R, [AREA.index(T) + 1])
            area.add_features(zn, R_LOOSE)
            area.abort()
        finally:
            area.destroy()
    return Scene((x0, P0), call, (x0, P0), z, tl)


def _local_predict(pkg, st):
    area = st.local(AREA)
    try:
        area.predict(2.0, 0.05, 4.0, Q, 0.025)
        area.close()
    finally:
        area.destroy()


LOCAL_IDS = list(range(41, N + 1))


def _local_own_build(dtype):
    """The gating of the LOCAL handle: primed after open, then the area's own update (T moved 34 m) and add_features."""
    xg, Pg = base(var={T: 4.0})
    s = CR.index_map(N, LOCAL_IDS)
    x0, P0 = xg[s], Pg[np.ix_(s, s)]
    t = LOCAL_IDS.index(T) + 1
    zu = obs(x0, t, MOVE * 4.01 / 4.0).reshape(2, 1)
    zn = np.array([[75.0], [2.2]])
    x1, P1 = O.update_sparse(x0, P0, zu, R, np.array([t]))
    x1, P1 = O.add_features_sparse(x1, P1, zn, R)
    z, tl = observations(x1, [LOCAL_IDS.index(j) + 1 for j in (44, 70)], [(t, 0.05, "c")])

    def call(pkg, st, mode):
        area = st.local(LOCAL_IDS)
        try:
            area.state.set_gate_mode(mode)
            area.state.associate_vector(z, R, GATE1, GATE2)                # primed: the local handle has a grid and a bound
            assert area.state.gate_info()["form"] == mode
            area.update(zu, R, [t])
            area.add_features(zn, R)
        except Exception:
            area.destroy()
            raise

        def close():
            area.abort()
            area.destroy()
        return {"query": area.state, "close": close}
    return Scene((xg, Pg), call, (x1, P1), z, tl, x_old=x0)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
ROWS = [
    # product library
    Row("set_state", "product", ["slam_ekf_set_state"], "abc", _replaced(_set_state), "forced", True),
    Row("set_state_device", "product", ["slam_ekf_set_state_device"], "abc", _replaced(_set_state_device), "forced", True),
    Row("raw write + state_written", "product", ["slam_ekf_state_written"], "abc", _raw_build, "forced", True),
    Row("update", "product", ["slam_ekf_update"], "c", _moved(lambda x, P, z, i: O.update_sparse(x, P, z, R, np.asarray(i)), _update()), "kept"),
    Row("update, async", "product", ["slam_ekf_update"], "c",
        _moved(lambda x, P, z, i: O.update_sparse(x, P, z, R, np.asarray(i)), _update(use_async=True)), "kept"),
    Row("update, joseph", "product", ["slam_ekf_update"], "c",
        _moved(lambda x, P, z, i: O.update_joseph_sparse(x, P, z, R, np.asarray(i)), _update(form="joseph")), "kept", True),
    Row("update, joseph: the bound is recomputed", "product", ["slam_ekf_update"], "r", _joseph_bound_build, "kept", True),
    # (the fold after 16 updates adds the slots up: 34 m is more than a quarter of a cell, so the fold rebuilds -- once)
    Row("17 updates between two queries", "product", ["slam_ekf_update"], "c", _many_updates(17), "forced"),
    Row("65 updates between two queries", "product", ["slam_ekf_update"], "c", _many_updates(65), "forced"),
    Row("add_features, loose R", "product", ["slam_ekf_augment"], "ab", _appended(O.add_features_sparse, lambda pkg, st, zn, Rn: st.add_features(zn, Rn)), "kept", tail=2),
    Row("add_features, loose R, bound invalid", "product", ["slam_ekf_augment"], "ab",
        _appended(O.add_features_sparse, lambda pkg, st, zn, Rn: st.add_features(zn, Rn), bound_invalid=True), "kept", True, tail=2),
    Row("observe", "product", ["slam_ekf_observe"], "c", _observe_build, "kept"),
    Row("remove_landmarks", "product", ["slam_ekf_remove_landmarks"], "c", _remove_build, "forced", True),
    Row("merge_landmarks", "product", ["slam_ekf_merge_landmarks"], "c", _merge_build, "forced", True),
    Row("predict", "product", ["slam_ekf_predict"], "control",
        _control(lambda x, P: O.predict_sparse(x, P, 2.0, 0.05, 4.0, Q, 0.025), lambda pkg, st: st.predict(2.0, 0.05, 4.0, Q, 0.025)), "kept",
        why="predict writes the pose, P_vv and P_vm only: no landmark mean, index or variance changes, and the gating reads the "
            "pose and P_vv from the state itself."),
    # frame
    Row("align", "frame", ["slam_ekf_transform"], "c", _align_build, "forced", True,
        why="(a)(b) cannot be reached with a factor of 2: a rotation raises the largest diagonal entry of a 2 x 2 block at most "
            "two-fold.  tests/test_gpu_ekf_transform.py::test_the_filter_goes_on_in_the_new_frame_variance_turned_onto_an_axis is "
            "the designed scene for the bound (1.95-fold, a decision between the gates)."),
    # join
    Row("join", "join", ["slam_ekf_join"], "ab", _join_build(False), "forced", True,
        why="(c) cannot be reached: join appends -- no existing landmark changes its index or its mean, and the query takes the "
            "pose from the state -- so every stale item is still right and the appended landmarks are read from the tail."),
    # (join, find_duplicates, merge: two calls that force and no query in between -- one rebuild at the next query)
    Row("join, merge_gate", "join", ["slam_ekf_join"], "ab", _join_build(True), "forced", True),
    # copy
    Row("copy_from", "copy", ["slam_ekf_copy"], "abc", _from_other(False), "forced", True),
    Row("select_from", "copy", ["slam_ekf_select"], "abc", _from_other(True), "forced", True),
    Row("reserve", "copy", ["slam_ekf_copy"], "control", _control(lambda x, P: (x, P), lambda pkg, st: st.reserve(2 * CAP)), None,
        why="reserve copies the state bit for bit into a fresh handle, whose bound and grid are still to be made; the gate mode is "
            "re-applied by the Python object.  (The fresh handle counts its rebuilds from zero: not compared.)"),
    # handover
    Row("pf_to_ekf", "handover", ["slam_pf_to_ekf"], "abc", _handover_build, "forced", True),
    # linear
    Row("fix_landmark", "linear", ["slam_ekf_update_linear"], "c", _fix_landmark_build, "forced"),
    Row("constrain_landmarks", "linear", ["slam_ekf_update_linear"], "c", _constrain_build, "forced"),
    Row("predict_linear", "linear", ["slam_ekf_predict_linear"], "control",
        _control(lambda x, P: LR.predict_linear(x, P, XV, GV, QV), lambda pkg, st: st.predict_linear(XV, GV, QV)), "kept",
        why="as predict: the pose, P_vv and P_vm only."),
    Row("predict_odometry", "linear", ["slam_ekf_predict_odometry"], "control",
        _control(lambda x, P: LR.predict_odometry(x, P, ODO, QV), lambda pkg, st: st.predict_odometry(ODO, QV)), "kept",
        why="as predict: the pose, P_vv and P_vm only."),
    # iterated
    Row("update_iterated", "iterated", ["slam_ekf_update_iterated"], "c",
        _moved(lambda x, P, z, i: IR.update(x, P, z, R, np.asarray(i))[0:2], lambda pkg, st, z, i: st.update_iterated(z, R, i)), "forced"),
    Row("observe_iterated", "iterated", ["slam_ekf_update_iterated"], "c", _observe_iterated_build, "forced"),
    # fej
    Row("FirstEstimates.update", "fej", ["slam_ekf_fej_update"], "c", _moved(_fej_ref(FR.update), _with_fej("update")), "forced"),
    Row("FirstEstimates.add_features, loose R", "fej", ["slam_ekf_fej_augment"], "ab", _appended(_fej_add_ref, _fej_add), "kept", tail=2),
    Row("FirstEstimates.predict", "fej", ["slam_ekf_fej_predict"], "control", _control(_fej_predict_ref, _fej_predict), "kept",
        why="as predict: the pose, P_vv and P_vm only (the vehicle Jacobian is taken elsewhere, the entries written are the same)."),
    Row("FirstEstimates.observe", "fej", ["slam_ekf_fej_update", "slam_ekf_fej_augment"], "c", _fej_observe_build, "forced"),
    # wide
    Row("FirstEstimates.update_joint", "wide", ["slam_ekf_wide_update"], "c", _moved(_fej_ref(WR.update), _with_fej("update_joint")), "forced"),
    Row("update_joint_at_estimates", "wide", ["slam_ekf_wide_update"], "c",
        _moved(lambda x, P, z, i: WR.update_at_estimates(x, P, z, R, np.asarray(i))[0:2],
               lambda pkg, st, z, i: st.update_joint_at_estimates(z, R, i)), "forced"),
    # local
    Row("LocalArea.close", "local", ["slam_ekf_local_open", "slam_ekf_local_update", "slam_ekf_local_augment", "slam_ekf_local_close"],
        "abc", _local_close_build, "forced", True),
    Row("LocalArea.abort", "local", ["slam_ekf_local_abort"], "control", _local_abort_build, "kept",
        why="an aborted area never wrote the global state: the local handle took its own copy at open."),
    Row("LocalArea.predict", "local", ["slam_ekf_local_predict"], "control",
        _control(lambda x, P: O.predict_sparse(x, P, 2.0, 0.05, 4.0, Q, 0.025), _local_predict), "forced",
        why="as predict, on the local handle; close then carries the pose, P_vv and P_vm over and no landmark changes."),
    # (the local handle is the product's: its update records the displacement, its augment leaves a tail of one)
    Row("LocalArea: its own gating", "local", ["slam_ekf_local_update", "slam_ekf_local_augment"], "c", _local_own_build, "kept"),
]

#: entry points that take an EKF handle (or an object attached to one) and leave the map as it is
READ_ONLY = {
    # lifetime and configuration
    "slam_ekf_create", "slam_ekf_destroy", "slam_ekf_set_gate_mode", "slam_ekf_set_async", "slam_ekf_sync", "slam_ekf_timing",
    "slam_ekf_timing_read", "slam_ekf_timing_reset", "slam_ekf_timing_min", "slam_ekf_timing_stats", "slam_ekf_debug_stamps",
    "slam_ekf_copy_floor",
    # reads of the state
    "slam_ekf_get_state", "slam_ekf_get_block", "slam_ekf_get_diag", "slam_ekf_get_landmark_blocks", "slam_ekf_gate_info",
    "slam_ekf_get_pose", "slam_ekf_num_landmarks", "slam_ekf_dtype", "slam_ekf_device_ptrs", "slam_ekf_associate", "slam_ekf_nis",
    "slam_ekf_predict_observation", "slam_ekf_ellipses", "slam_ekf_find_duplicates", "slam_ekf_capacity", "slam_ekf_to_pf",
    "slam_ekf_linear_nis", "slam_ekf_iterated_nis", "slam_ekf_iterated_limits", "slam_ekf_wide_nis", "slam_ekf_wide_limits",
    # the joint-compatibility workspace and the factor object: they read the state
    "slam_ekf_jc_create", "slam_ekf_jc_destroy", "slam_ekf_associate_joint", "slam_ekf_joint_nis",
    "slam_ekf_factor_create", "slam_ekf_factor_destroy", "slam_ekf_factor_compute", "slam_ekf_factor_info", "slam_ekf_factor_get",
    "slam_ekf_factor_mean", "slam_ekf_factor_solve", "slam_ekf_factor_multiply",
    # the first-estimates object: these write ITS linearisation points, never x or P
    "slam_ekf_fej_create", "slam_ekf_fej_destroy", "slam_ekf_fej_reset", "slam_ekf_fej_remap", "slam_ekf_fej_transform",
    "slam_ekf_fej_get", "slam_ekf_fej_set", "slam_ekf_fej_limits",
    # the local area: lifetime and reads
    "slam_ekf_local_create", "slam_ekf_local_destroy", "slam_ekf_local_state", "slam_ekf_local_info", "slam_ekf_local_get",
}


def by_name(name):
    return next(r for r in ROWS if r.name == name)
