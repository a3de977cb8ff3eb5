"""Host side of the FastSLAM map read-out (no GPU): the NumPy finalisation of the map sums (slam.jl_amd/pf.py:
finalise_map, the arithmetic slam_pf_get_map does in C), the ellipse convention, and telemetry.monitor_messages on an
object with the PFSlamState read-out methods."""
import math

import numpy as np
import pytest


def sums_of(w, m, P, used=None):
    """Rows of map_sums for ONE landmark in fp64: w [n], m [n, 2], P [n, 3] (Pxx, Pxy, Pyy)."""
    w, m, P = np.asarray(w, float), np.asarray(m, float), np.asarray(P, float)
    u = np.ones(len(w), bool) if used is None else np.asarray(used, bool)
    wu = np.where(u, w, 0.0)
    pose_row = [w.sum(), 0, 0, 0, 0, 0, 0, w.sum(), 0, len(w)]
    row = [wu.sum(), (wu * m[:, 0]).sum(), (wu * m[:, 1]).sum(), (wu * m[:, 0] ** 2).sum(), (wu * m[:, 0] * m[:, 1]).sum(),
           (wu * m[:, 1] ** 2).sum(), (wu * P[:, 0]).sum(), (wu * P[:, 1]).sum(), (wu * P[:, 2]).sum(), u.sum()]
    return np.array([pose_row, row], dtype=np.float64)


def test_finalisation_on_hand_derived_cases(pkg):
    # two particles, weights 1/4 and 3/4, means (0, 0) and (4, 0), P = diag(1, 1): mean (3, 0), C = [[1 + 3, 0], [0, 1]]
    s = sums_of([0.25, 0.75], [[0, 0], [4, 0]], [[1, 0, 1], [1, 0, 1]])
    out = pkg.pf.finalise_map(s)
    assert out.shape == (1, 8)
    assert out[0].tolist() == pytest.approx([1.0, 3.0, 0.0, 4.0, 0.0, 1.0, 2.0, 0.0], abs=1e-15)
    # only the second particle holds the landmark: mass 3/4, its own Gaussian
    s = sums_of([0.25, 0.75], [[0, 0], [4, 0]], [[0, 0, 0], [2, 0.5, 1]], used=[False, True])
    assert pkg.pf.finalise_map(s)[0].tolist() == pytest.approx([0.75, 4.0, 0.0, 2.0, 0.5, 1.0, 1.0, 0.0], abs=1e-15)
    # a landmark with mass 0 is a row of zeros, next to one with mass
    both = np.vstack([s, np.zeros((1, 10))])
    out = pkg.pf.finalise_map(both)
    assert out.shape == (2, 8) and not out[1].any() and out[0, 0] == 0.75
    # unnormalised weights give the same map
    assert np.allclose(pkg.pf.finalise_map(sums_of([1.0, 3.0], [[0, 0], [4, 0]], [[1, 0, 1], [1, 0, 1]])),
                       [[1.0, 3.0, 0.0, 4.0, 0.0, 1.0, 2.0, 0.0]], atol=1e-15)


def test_sums_of_two_ranks_add_up_to_the_union(pkg):
    rng = np.random.default_rng(3)
    n = 200
    w = rng.uniform(0.1, 1.0, n)
    m = rng.normal([5.0, -3.0], 0.3, (n, 2))
    P = np.abs(rng.normal(0.05, 0.01, (n, 3)))
    used = rng.uniform(size=n) < 0.8
    whole = sums_of(w, m, P, used)
    a, b = sums_of(w[:70], m[:70], P[:70], used[:70]), sums_of(w[70:], m[70:], P[70:], used[70:])
    assert np.allclose(a + b, whole, rtol=1e-14)
    assert np.allclose(pkg.pf.finalise_map(a + b), pkg.pf.finalise_map(whole), rtol=1e-12, atol=1e-14)
    # and the finalisation is the mixture's moments
    wu = np.where(used, w, 0.0)
    mean = (wu[:, None] * m).sum(0) / wu.sum()
    d = m - mean
    cxx = (wu * (P[:, 0] + d[:, 0] ** 2)).sum() / wu.sum()
    cxy = (wu * (P[:, 1] + d[:, 0] * d[:, 1])).sum() / wu.sum()
    got = pkg.pf.finalise_map(whole)[0]
    assert got[1:3].tolist() == pytest.approx(mean.tolist(), rel=1e-13)
    assert got[3] == pytest.approx(cxx, rel=1e-9) and got[4] == pytest.approx(cxy, rel=1e-9, abs=1e-12)
    assert got[0] == pytest.approx(wu.sum() / w.sum(), rel=1e-14) and got[6] == used.sum()


def test_ellipse_convention(pkg):
    """rx <= ry, phi of the first (smaller eigenvalue's) eigenvector in [-pi/2, pi/2] (slam_ekf_ellipses)."""
    E = pkg.pf.ellipse_axes
    rx, ry, phi = E(np.array([1.0, 4.0]), np.array([0.0, 0.0]), np.array([4.0, 1.0]))       # diagonal
    assert rx.tolist() == [1.0, 1.0] and ry.tolist() == [2.0, 2.0]
    assert phi[0] == pytest.approx(0.0) and abs(phi[1]) == pytest.approx(math.pi / 2)
    c, s = math.cos(math.pi / 4), math.sin(math.pi / 4)                                       # diag(1, 4) rotated by 45 degrees
    Rm = np.array([[c, -s], [s, c]])
    Cm = Rm @ np.diag([1.0, 4.0]) @ Rm.T
    rx, ry, phi = E(Cm[0, 0], Cm[0, 1], Cm[1, 1])
    assert float(rx) == pytest.approx(1.0) and float(ry) == pytest.approx(2.0) and float(phi) == pytest.approx(math.pi / 4)
    Cm = Rm.T @ np.diag([1.0, 4.0]) @ Rm                                                      # ... by -45 degrees
    assert float(E(Cm[0, 0], Cm[0, 1], Cm[1, 1])[2]) == pytest.approx(-math.pi / 4)
    rx, ry, phi = E(2.0, 0.0, 2.0)                                                            # a circle
    assert float(rx) == float(ry) == pytest.approx(math.sqrt(2.0)) and -math.pi / 2 <= float(phi) <= math.pi / 2
    # against numpy's eigen-decomposition on random matrices
    rng = np.random.default_rng(0)
    for _ in range(50):
        A = rng.normal(size=(2, 2))
        Cm = A @ A.T
        lam, vec = np.linalg.eigh(Cm)
        rx, ry, phi = E(Cm[0, 0], Cm[0, 1], Cm[1, 1])
        assert float(rx) == pytest.approx(math.sqrt(lam[0]), rel=1e-9) and float(ry) == pytest.approx(math.sqrt(lam[1]), rel=1e-9)
        v = vec[:, 0] * (1 if vec[0, 0] >= 0 else -1)
        assert abs(math.cos(float(phi)) * v[1] - math.sin(float(phi)) * v[0]) < 1e-7          # parallel
        assert -math.pi / 2 <= float(phi) <= math.pi / 2


class _StubPF:
    """A PFSlamState over fixed map sums (what the device would return): only the queries are replaced."""
    def __init__(self, pkg, sums):
        self._base, self._s, self.queries = pkg.PFSlamState, sums, 0

    def map_sums(self, ids=None):
        self.queries += 1
        return self._s[:1] if ids is not None and len(ids) == 0 else self._s

    def __getattr__(self, name):                     # the read-out methods themselves are PFSlamState's
        attr = getattr(self._base, name)
        return attr.fget(self) if isinstance(attr, property) else attr.__get__(self)


def test_monitor_messages_accepts_the_particle_filter_read_outs(pkg):
    w = np.array([0.25, 0.75])
    x, y, phi = np.array([1.0, 3.0]), np.array([2.0, 2.0]), np.array([0.1, 0.1])
    pose_row = [w.sum(), (w * x).sum(), (w * y).sum(), (w * x * x).sum(), (w * x * y).sum(), (w * y * y).sum(),
                (w * np.sin(phi)).sum(), (w * np.cos(phi)).sum(), 0.0, 2.0]
    lm1 = sums_of(w, [[0, 0], [4, 0]], [[1, 0, 1], [1, 0, 1]])[1]
    sums = np.array([pose_row, lm1, np.zeros(10), lm1])                # landmark 2 was never seen
    st = _StubPF(pkg, sums)
    assert st.N == 2
    assert st.pose().tolist() == pytest.approx([2.5, 2.0, 0.1])
    fe = st.feature_ellipses()
    assert fe.shape == (5, 2) and fe[:, 0].tolist() == pytest.approx([3.0, 0.0, 1.0, 2.0, math.pi / 2])
    ve = st.vehicle_ellipse()
    assert ve.tolist() == pytest.approx([2.5, 2.0, 0.1, 0.0, math.sqrt(0.75), math.pi / 2], abs=1e-12)
    msgs = pkg.telemetry.monitor_messages(st, [2.4, 2.0, 0.1], st.pose(), z=np.array([[5.0], [0.2]]), state_updated=True, timestamp=1.0)
    assert [m["type"] for m in msgs] == ["tracks", "state", "lidar", "feature-ellipses", "vehicle-ellipse"]
    assert msgs[3]["data"][1] == {"cx": 3.0, "cy": 0.0, "rx": 1.0, "ry": 2.0, "phi": pytest.approx(math.pi / 2)}
    assert set(msgs[4]["data"][0]) == {"cx", "cy", "vehicle_phi", "rx", "ry", "phi"}
    assert pkg.telemetry.to_json(msgs[3])
    # one snapshot serves a whole message set from ONE query and gives the same messages
    st.queries = 0
    snap = st.snapshot()
    again = pkg.telemetry.monitor_messages(snap, [2.4, 2.0, 0.1], snap.pose(), z=np.array([[5.0], [0.2]]), state_updated=True, timestamp=1.0)
    assert st.queries == 1 and pkg.telemetry.to_json(again[1:]) == pkg.telemetry.to_json(msgs[1:])
