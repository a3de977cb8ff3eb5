"""What the gating keeps beside x and P -- the packed diagonal blocks, the variance bound, the grid over the landmark means
(csrc/common.h, struct slam_ekf) -- after every call that changes the map (tests/gate_cache_scenes.py: one row per call), on
handles that were PRIMED first: a grid exists, it is live, the bound is valid.  Most other tests call into a fresh handle, where
everything is still forced.  Each row's scene is one where the side state of before the call would decide differently
(tests/test_gate_cache_cpu.py shows that from the fp64 references); here the decisions of the grid form, of the sweep with the
pre-gate always on (SLAMHIP_X=64) and of the plain sweep (SLAMHIP_X=32: the control) must be the oracle's on the state as the
device holds it, and those of a fresh handle the state was uploaded into; where a row says so, the grid handle's rebuild count,
its tail, and -- for the call that has to make the bound SMALLER again -- the number of landmarks its query evaluated.  Then one seeded sequence of the table's calls on one
primed grid handle and one plain-sweep handle."""
import numpy as np
import pytest

from oracle import ekf_ref as O
from tests import gate_cache_ref as GR
from tests import gate_cache_scenes as S
from tests.strip_ref import check_storage
from tests.test_gpu_ekf import DTYPES, rounded

pytestmark = pytest.mark.gpu

HANDLES = (("grid", "grid", None), ("pre", "sweep", "64"), ("plain", "sweep", "32"))      # name, gate mode, SLAMHIP_X at creation


def _env(monkeypatch, flag):
    if flag is None:
        monkeypatch.delenv("SLAMHIP_X", raising=False)
    else:
        monkeypatch.setenv("SLAMHIP_X", flag)


def _oracle(st, z):
    x, P = rounded(st)
    nis, nd = O.association_table_sparse(x, P, z, S.R)
    return O.assoc_vector(nis, nd, S.GATE1, S.GATE2)


def _query(st, z):
    return st.associate_vector(z, S.R, S.GATE1, S.GATE2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row", S.ROWS, ids=[r.name for r in S.ROWS])
def test_the_gating_follows_the_call_on_primed_handles(pkg, monkeypatch, row, dtype):
    sc = row.build(dtype)
    z_prime = S.observations(sc.before[0], S.MATCH, [])[0]
    got, closers = {}, []
    try:
        for name, mode, flag in HANDLES:
            what = f"{row.name} {dtype} {name}"
            _env(monkeypatch, flag)                    # (a call that makes a handle of its own makes it under the same switch)
            st = pkg.EKFSlamState(*sc.before, dtype=dtype, max_landmarks=S.CAP)
            closers.append(st.close)
            st.set_gate_mode(mode)
            # primed: a grid exists and is live, the bound is valid
            assert np.array_equal(_query(st, z_prime), _oracle(st, z_prime)), what
            info = st.gate_info()
            assert info["form"] == mode and (mode != "grid" or (info["rebuilds"] == 1 and info["in_grid"] == S.N)), (what, info)
            built = rounded(st)[0][3:]                 # the means the grid's items carry
            out = sc.call(pkg, st, mode)
            q = st
            if isinstance(out, dict):             # (most calls return what the library call returned)
                q = out["query"]
                closers.insert(0, out["close"])
            i0 = q.gate_info()
            r0 = i0["rebuilds"]
            want = _oracle(q, sc.z)
            for i, j, _conds in sc.targets:            # the designed decisions survive the device's rounding
                assert want[i] == j, (what, i, j, want.tolist())
            assert np.any(want > 0) and np.any(want < 0), what
            got[name] = _query(q, sc.z)
            assert np.array_equal(got[name], want), (what, got[name].tolist(), want.tolist())
            info = q.gate_info()
            assert info["form"] == mode, (what, info)
            if mode == "grid" and row.rebuild is not None:
                assert info["rebuilds"] - r0 == (1 if row.rebuild == "forced" else 0), (what, row.rebuild, r0, info)
            if mode == "grid" and row.tail is not None:        # the appended landmarks are read from the tail, the grid is as built
                assert info["in_grid"] == S.N and info["tail"] == row.tail, (what, info)
            if mode == "grid" and row.sensitive != "control" and "r" in row.sensitive:
                # the bound was recomputed: the query evaluated no more than the reach of the matrix's own largest variance allows
                x, P = rounded(q)
                drift = float(np.max(np.abs(x[3:] - built))) * (1.0 + 1e-6) + 1e-12
                most = sum(GR.evaluated_bounds(x, P, sc.z[:, i], built, GR.true_pmax(P), S.R, S.GATE2, drift)[1] for i in range(sc.z.shape[1]))
                stale = sum(GR.evaluated_bounds(x, P, sc.z[:, i], built, sc.stale_bound, S.R, S.GATE2)[0] for i in range(sc.z.shape[1]))
                done = info["evaluated"] - i0["evaluated"]
                print(f"{what}: evaluated {done}; at most {most} under the recomputed bound, at least {stale} under the old one")
                assert 1 <= done <= most < stale, (what, done, most, stale)
            xg, Pg = q.download()
            fresh = pkg.EKFSlamState(xg, Pg, dtype=dtype, max_landmarks=q.capacity)
            closers.insert(0, fresh.close)
            fresh.set_gate_mode(mode)
            assert np.array_equal(_query(fresh, sc.z), want), what
            assert fresh.gate_info()["form"] == mode, what
            check_storage(q, pkg, Pg, what=what)
        assert np.array_equal(got["grid"], got["pre"]) and np.array_equal(got["grid"], got["plain"]), (row.name, got)
    finally:
        monkeypatch.delenv("SLAMHIP_X", raising=False)
        for fn in closers:
            fn()


# ---- one sequence of the table's calls -------------------------------------------------------------------------------------------------
def _noisy(rng, x, ids):
    return np.stack([S.obs(x, j, *rng.normal(0.0, [0.03, 0.003])) for j in ids], axis=1)


def _ids(rng, x, count):
    return rng.choice(np.arange(1, (len(x) - 3) // 2 + 1), size=count, replace=False)


def _free_spot(x, k):
    """An observation of nothing: beyond every landmark, on its own bearing."""
    far = np.max(np.hypot(x[3::2] - x[0], x[4::2] - x[1])) if len(x) > 3 else 0.0
    return np.array([far + 15.0 + 9.0 * k, -2.5 + 0.7 * k])


def _fej(st, fn):
    obj = st.fej()
    try:
        fn(obj)
    finally:
        obj.close()


def _area(st, ids, fn):
    area = st.local(ids)
    try:
        fn(area)
    finally:
        area.destroy()


def _op_update(form="cholesky"):
    def prep(rng, x, P):
        ids = _ids(rng, x, 3)
        return _noisy(rng, x, ids), ids
    return prep, lambda pkg, st, a: st.update(a[0], S.R, a[1], form=form)


def _op_many_updates(count):
    def prep(rng, x, P):
        return [(_noisy(rng, x, [j]), [j]) for j in _ids(rng, x, count)]

    def apply(pkg, st, a):
        for z, ids in a:
            st.update(z, S.R, ids)
    return prep, apply


def _op_add(R):
    def prep(rng, x, P):
        return np.stack([_free_spot(x, 0), _free_spot(x, 1)], axis=1)
    return prep, lambda pkg, st, a: st.add_features(a, R)


def _op_observe():
    def prep(rng, x, P):
        return np.concatenate([_noisy(rng, x, _ids(rng, x, 4)), _free_spot(x, 2).reshape(2, 1)], axis=1)
    return prep, lambda pkg, st, a: st.observe(a, S.R, S.GATE1, S.GATE2)


def _op_remove():
    return (lambda rng, x, P: np.sort(_ids(rng, x, 2))), lambda pkg, st, a: st.remove_landmarks(a)


def _op_duplicate_then_merge():
    """A landmark entered twice (add_features of its own exact observation), then merged away."""
    def prep(rng, x, P):
        j = int(_ids(rng, x, 1)[0])
        return j, S.obs(x, j).reshape(2, 1), (len(x) - 3) // 2 + 1

    def apply(pkg, st, a):
        st.add_features(a[1], S.R)
        st.merge_landmarks([(a[0], a[2])])
    return prep, apply


def _op_fix():
    def prep(rng, x, P):
        j = int(_ids(rng, x, 1)[0])
        return j, x[S.f(j):S.f(j) + 2] + rng.normal(0.0, 0.02, 2)
    return prep, lambda pkg, st, a: st.fix_landmark(a[0], a[1], 0.01 * np.eye(2))


def _op_constrain():
    def prep(rng, x, P):
        a, b = (int(j) for j in _ids(rng, x, 2))
        return a, b, x[S.f(b):S.f(b) + 2] - x[S.f(a):S.f(a) + 2] + rng.normal(0.0, 0.02, 2)
    return prep, lambda pkg, st, a: st.constrain_landmarks(a[0], a[1], a[2], 0.01 * np.eye(2))


def _op_iterated():
    def prep(rng, x, P):
        ids = _ids(rng, x, 3)
        return _noisy(rng, x, ids), ids
    return prep, lambda pkg, st, a: st.update_iterated(a[0], S.R, a[1])


def _op_fej(method, count):
    def prep(rng, x, P):
        ids = _ids(rng, x, count)
        return _noisy(rng, x, ids), ids
    return prep, lambda pkg, st, a: _fej(st, lambda obj: getattr(obj, method)(a[0], S.R, a[1]))


def _op_fej_add():
    def prep(rng, x, P):
        return _free_spot(x, 3).reshape(2, 1)
    return prep, lambda pkg, st, a: _fej(st, lambda obj: obj.add_features(a, S.R_LOOSE))


def _op_joint_at_estimates():
    def prep(rng, x, P):
        ids = _ids(rng, x, 9)
        return _noisy(rng, x, ids), ids
    return prep, lambda pkg, st, a: st.update_joint_at_estimates(a[0], S.R, a[1])


def _op_join():
    def prep(rng, x, P):
        xB = np.array([0.5, -0.3, 0.04, 95.0, 20.0, -90.0, 35.0])
        return xB, np.diag([1e-6, 1e-6, 1e-8, 0.5, 0.5, 0.5, 0.5])

    def apply(pkg, st, a):
        sub = st.submap(8)
        try:
            sub.set_state(*a)
            st.join(sub)
        finally:
            sub.close()
    return prep, apply


def _op_local(close):
    def prep(rng, x, P):
        ids = np.sort(_ids(rng, x, 6))
        return ids, _noisy(rng, x, ids[:2]), _free_spot(x, 4).reshape(2, 1)

    def apply(pkg, st, a):
        def steps(area):
            area.update(a[1], S.R, [1, 2])
            area.add_features(a[2], S.R)
            (area.close if close else area.abort)()
        _area(st, a[0], steps)
    return prep, apply


def _op_from_copy(select):
    def prep(rng, x, P):
        N = (len(x) - 3) // 2
        return np.delete(np.arange(N, 0, -1), [3, 11])                # every landmark but two, in descending order

    def apply(pkg, st, a):
        other = st.copy()
        try:
            other.predict(1.0, 0.02, 4.0, S.Q, 0.025)
            if select:
                st.select_from(other, a)
            else:
                st.copy_from(other)
            st.sync()
        finally:
            other.close()
    return prep, apply


def _op_set_state():
    def prep(rng, x, P):
        x2, P2 = x.copy(), P.copy()
        x2[3:] += rng.normal(0.0, 0.5, len(x) - 3)
        P2[np.arange(3, len(x)), np.arange(3, len(x))] *= 1.5
        return x2, P2
    return prep, lambda pkg, st, a: st.set_state(*a)


SEQUENCE = [
    ("update", _op_update()), ("predict", (lambda rng, x, P: None, lambda pkg, st, a: st.predict(2.0, 0.05, 4.0, S.Q, 0.025))),
    ("add_features", _op_add(S.R)), ("update, joseph", _op_update("joseph")), ("observe", _op_observe()),
    ("remove_landmarks", _op_remove()), ("add_features, loose R", _op_add(S.R_LOOSE)), ("update", _op_update()),
    ("merge_landmarks", _op_duplicate_then_merge()), ("fix_landmark", _op_fix()), ("constrain_landmarks", _op_constrain()),
    ("predict_odometry", (lambda rng, x, P: None, lambda pkg, st, a: st.predict_odometry(S.ODO, S.QV))),
    ("update_iterated", _op_iterated()), ("FirstEstimates.update", _op_fej("update", 3)), ("FirstEstimates.add_features", _op_fej_add()),
    ("FirstEstimates.predict", (lambda rng, x, P: None, lambda pkg, st, a: _fej(st, lambda obj: obj.predict(2.0, -0.05, 4.0, S.Q, 0.025)))),
    ("FirstEstimates.update_joint", _op_fej("update_joint", 12)), ("update_joint_at_estimates", _op_joint_at_estimates()),
    ("transform", (lambda rng, x, P: None, lambda pkg, st, a: st.transform(30.0, -12.0, 0.8))), ("join", _op_join()),
    ("LocalArea.close", _op_local(True)), ("LocalArea.abort", _op_local(False)), ("17 updates", _op_many_updates(17)),
    ("copy_from", _op_from_copy(False)), ("select_from", _op_from_copy(True)), ("remove_landmarks", _op_remove()),
    ("add_features", _op_add(S.R)), ("set_state", _op_set_state()), ("update", _op_update()),
    ("predict_linear", (lambda rng, x, P: (x[0:3] + [0.3, -0.2, 0.02],), lambda pkg, st, a: st.predict_linear(a[0], S.GV, S.QV))),
    ("reserve", (lambda rng, x, P: None, lambda pkg, st, a: st.reserve(2 * S.CAP))), ("update", _op_update()),
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_sequence_of_the_calls_on_a_primed_grid_handle_and_a_plain_sweep(pkg, monkeypatch, dtype):
    """Every call of SEQUENCE on both handles with the same arguments, a query after each: the two vectors are equal and are the
    oracle's on the state as the device holds it, at every step; at the end the two states are bit-identical."""
    rng = np.random.default_rng(7100)
    x0, P0 = S.base(var={S.T: 4.0, 31: 0.04})
    sts = {}
    try:
        for name, mode, flag in (HANDLES[0], HANDLES[2]):
            _env(monkeypatch, flag)
            sts[name] = pkg.EKFSlamState(x0, P0, dtype=dtype, max_landmarks=S.CAP)
            sts[name].set_gate_mode(mode)
        monkeypatch.delenv("SLAMHIP_X", raising=False)
        for step, (label, (prep, apply)) in enumerate([("prime", (lambda rng, x, P: None, lambda pkg, st, a: None))] + SEQUENCE):
            what = f"{dtype} step {step} ({label})"
            x, P = rounded(sts["grid"])
            args = prep(rng, x, P)
            for st in sts.values():
                apply(pkg, st, args)
            x, P = rounded(sts["grid"])
            ids = _ids(rng, x, 6)
            z = np.concatenate([_noisy(rng, x, ids), _noisy(rng, x, ids[:2]) + [[0.45], [0.0]], _free_spot(x, 5).reshape(2, 1)], axis=1)
            nis, nd = O.association_table_sparse(x, P, z, S.R)
            want = O.assoc_vector(nis, nd, S.GATE1, S.GATE2)
            got = {name: _query(st, z) for name, st in sts.items()}
            assert np.array_equal(got["grid"], want) and np.array_equal(got["plain"], want), (what, got, want.tolist())
            assert sts["grid"].gate_info()["form"] == "grid" and sts["plain"].gate_info()["form"] == "sweep", what
            assert np.any(want > 0) and want[-1] == -1, (what, want.tolist())
        (xa, Pa), (xb, Pb) = sts["grid"].download(), sts["plain"].download()
        assert xa.tobytes() == xb.tobytes() and np.ascontiguousarray(Pa).tobytes() == np.ascontiguousarray(Pb).tobytes()
        check_storage(sts["grid"], pkg, Pa, what=f"{dtype} after the sequence")
    finally:
        monkeypatch.delenv("SLAMHIP_X", raising=False)
        for st in sts.values():
            st.close()
