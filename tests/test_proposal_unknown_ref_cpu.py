"""FastSLAM 2.0 with unknown correspondences (slam_pf_step_proposal_unknown / slam_pf_associate_proposal,
include/ext/slamhip_proposal.h), the parts that need no GPU: tests/proposal_unknown_ref.py against the oracle's predict,
update_unknown and step_proposal; the conditions of the scene the GPU test runs; what is particular to this library's surface (the
checks every side library shares are made from its row of the table by tests/test_companions_cpu.py); and the status codes that
are decided before a device is touched."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import pf_ref as O
from tests import abi_surface as ABI
from tests import proposal_unknown_ref as P

HEADER = os.path.join(ABI.INCLUDE, "ext", "slamhip_proposal.h")
NAMES = {"slam_pf_step_proposal_unknown", "slam_pf_associate_proposal", "slam_pf_proposal_limits"}
QFULL = np.array([[0.25, 0.004], [0.004, math.radians(3.0) ** 2]])


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---- the model against the existing oracle ------------------------------------------------------------------------------------------
def test_without_observations_the_step_is_predict_bit_for_bit():
    a, b = P.fresh(n=300), P.fresh(cls=O.OraclePF, n=300)
    for t in range(3):
        dec = a.step_proposal_unknown(P.V, P.steer(t), P.WHEELBASE, P.Q, P.DT, np.zeros((2, 0)), P.R, P.GATE1, P.GATE2)
        b.predict(P.V, P.steer(t), P.WHEELBASE, P.Q, P.DT)
        assert dec.shape == (0, 300)
        assert _same(a.pose, b.pose) and _same(a.logw, b.logw) and _same(a.lm, b.lm) and a.step == b.step == t + 1


def test_on_a_cleared_map_every_observation_is_new_and_the_step_is_predict_and_update_unknown_bit_for_bit():
    a, b = P.fresh(n=300), P.fresh(cls=O.OraclePF, n=300)
    G, z = P.scene(1)[0]
    dec = a.step_proposal_unknown(P.V, G, P.WHEELBASE, P.Q, P.DT, z, P.R, P.GATE1, P.GATE2)
    b.predict(P.V, G, P.WHEELBASE, P.Q, P.DT)
    ref = b.update_unknown(z, P.R, P.GATE1, P.GATE2)
    assert (dec == -1).all() and _same(dec, ref)
    assert _same(a.pose, b.pose) and _same(a.lm, b.lm) and _same(a.logw, b.logw)
    assert (a.lm[:4, 2] >= 0).all() and (a.lm[4:, 2] == -1).all()


def test_with_wide_gates_on_separated_landmarks_the_step_is_the_known_id_proposal():
    n = 257
    ids = np.array([1, 3, 6, 3, 2])                                      # landmark 3 observed twice
    lms = P.LANDMARKS[:6]
    a, b = P.ProposalUnknownPF(n, 6, 3), O.OraclePF(n, 6, 3)
    rng = np.random.default_rng(4)
    for pf in (a, b):
        pf.set_pose(P.START)
        pf.init_landmarks(lms, 0.04, 0.1)
    pose = np.array(P.START)
    z = np.zeros((2, len(ids)))
    for i, j in enumerate(ids):
        dx, dy = lms[j - 1] - pose[:2] - np.array([P.V * P.DT * math.cos(pose[2]), P.V * P.DT * math.sin(pose[2])])
        z[:, i] = [math.hypot(dx, dy) + 0.05 * rng.standard_normal(), math.atan2(dy, dx) - pose[2] + 0.008 * rng.standard_normal()]
    dec = a.step_proposal_unknown(P.V, 0.03, P.WHEELBASE, QFULL, P.DT, z, P.R, 1e6, 1e9)
    b.step_proposal(P.V, 0.03, P.WHEELBASE, QFULL, P.DT, z, ids, P.R)
    assert _same(dec, np.repeat((ids - 1)[:, None], n, axis=1))
    for got, want in ((a.pose, b.pose), (a.logw, b.logw), (a.lm, b.lm)):
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.max(np.abs(want))))
    assert a.step == b.step == 1 and not a.last_capacity.any()


def test_with_a_vanishing_control_noise_the_decisions_are_those_of_fastslam_1():
    q = P.Q * 1e-12
    d2, _, _ = P.run("2.0", q=q)
    d1, _, _ = P.run("1.0", q=q)
    assert all(_same(a, b) for a, b in zip(d2, d1))
    assert P.counts(d2) == P.counts(d1) and P.counts(d2)[1] == P.SLOTS * P.N


# ---- the scene, as conditions --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return P.run("2.0")


def test_the_scene_sees_the_pose_term(base):
    """Measured: 609 of 72 624 decisions differ without B B' in the association's S."""
    without, _, _ = P.run("2.0", pose_term=False)
    differ = sum(int((a != b).sum()) for a, b in zip(base[0], without))
    print("decisions that differ without the pose term:", differ)
    assert differ >= 100


def test_the_scene_has_few_decisions_at_a_gate_edge(base):
    """Measured: 5 decisions (5 particles) change with the gates scaled by 1.002, 5 (5 particles) with 0.998: 10 of 72 624
    decisions, 10 of 1513 particles (0.66 %)."""
    moved = np.zeros(P.N, dtype=bool)
    for scale in (1.002, 0.998):
        dec, _, _ = P.run("2.0", gate_scale=scale)
        for a, b in zip(base[0], dec):
            moved |= (a != b).any(axis=0)
        print("gates x", scale, ":", sum(int((a != b).sum()) for a, b in zip(base[0], dec)), "decisions;", int(moved.sum()),
              "particles so far")
    assert moved.sum() <= 0.01 * P.N


def test_the_proposal_keeps_more_effective_particles_than_fastslam_1(base):
    """Measured: mean Neff / n 0.378 against 0.093; 58 642 matches / 12 104 new / 1 878 dropped against 45 771 / 15 447 / 11 406."""
    d1, n1, _ = P.run("1.0")
    print("2.0:", P.counts(base[0]), float(np.mean(base[1])), " 1.0:", P.counts(d1), float(np.mean(n1)))
    assert sum(P.counts(base[0])) == sum(P.counts(d1)) == 4 * P.STEPS * P.N
    assert np.mean(base[1]) > np.mean(n1)
    assert P.counts(base[0])[0] > P.counts(d1)[0]


def test_a_ninth_landmark_exhausts_the_slots_and_is_reported_dropped():
    dec, _, pf = P.run("2.0", steps=P.scene(ninth_from=9))
    assert pf.last_capacity.any() and (dec[-1][pf.last_capacity] == -2).all()
    assert (pf.lm[:, 2] >= 0).all()
    assert (pf.last_nis[dec[-1] < 0] != pf.last_nis[dec[-1] < 0]).all() and np.isfinite(pf.last_nis[dec[-1] >= 0]).all()


# ---- the surface: the checks every library shares are tests/test_companions_cpu.py's, from this library's row of the table --------------
def test_what_is_particular_to_this_library(pkg):
    L = pkg._lib
    assert NAMES == set(L.proposal_lib.signatures)
    with open(ABI.JULIA) as f:
        src = f.read()
    for word in ("step_proposal_unknown!", "associate_proposal", "proposal_max_obs"):
        assert word in src.split("module SLAMHip")[1].split("const libslamhip =")[0], word      # exported
    with open(HEADER) as f:
        text = f.read()
    assert '#include "slamhip.h"' in text and "#define SLAM_PF_PROPOSAL_MAXOBS 16" in text
    assert L.proposal_max_obs() == 16 == P.MAXOBS                       # (slam_pf_proposal_limits needs no device)
    for word in ("step_proposal_unknown", "associate_proposal"):
        assert callable(getattr(pkg.pf.PFShard, word)), word


def test_bad_arguments_are_status_codes_without_a_device(pkg):
    """Every rule that needs no state is decided before the handle is read: the handle here is not one."""
    L = pkg._lib
    lib = L.proposal_lib()
    BAD = L.SLAM_E_BADARG
    fake = ctypes.c_void_p(0x1000)
    dbl = lambda *v: (ctypes.c_double * len(v))(*v)
    Qd, Rd = dbl(0.25, 0.0, 0.0, 0.0027), dbl(0.0025, 0.0, 0.0, 7.6e-5)
    z = dbl(*([10.0, 0.1] * 17))
    out = dbl(7.0, 7.0, 7.0)
    nan = float("nan")

    def step(h=fake, V=3.0, G=0.1, w=4.0, Q=Qd, dt=0.1, zz=z, m=4, R=Rd, g1=9.2, g2=25.0, o=out):
        return lib.slam_pf_step_proposal_unknown(h, V, G, w, Q, dt, zz, m, R, g1, g2, None, o)

    def assoc(h=fake, V=3.0, G=0.1, w=4.0, Q=Qd, dt=0.1, zz=z, m=4, R=Rd, g1=9.2, g2=25.0, o=None):
        return lib.slam_pf_associate_proposal(h, V, G, w, Q, dt, zz, m, R, g1, g2, None, None)

    for fn in (step, assoc):
        assert fn(h=None) == BAD and "null handle" in L.last_error()
        assert fn(Q=None) == BAD and fn(zz=None) == BAD and fn(R=None) == BAD
        assert fn(m=17) == BAD and "16" in L.last_error()
        assert fn(m=-1) == BAD
        for kw in ({"V": nan}, {"G": float("inf")}, {"w": nan}, {"dt": nan}, {"g1": nan}, {"g2": float("inf")}):
            assert fn(**kw) == BAD and "finite" in L.last_error(), kw
        assert fn(zz=dbl(10.0, nan, 3.0, 0.0), m=2) == BAD and "finite" in L.last_error()
        assert fn(Q=dbl(0.25, nan, 0.0, 0.1)) == BAD and fn(R=dbl(nan, 0.0, 0.0, 0.1)) == BAD
        assert fn(Q=dbl(0.25, 0.3, 0.3, 0.1)) == BAD and "positive definite" in L.last_error()       # det < 0
        assert fn(Q=dbl(-1.0, 0.0, 0.0, 0.1)) == BAD and "positive definite" in L.last_error()
    assert step(o=None) == BAD
    assert list(out) == [7.0] * 3
    assert lib.slam_pf_proposal_limits(None) == BAD
    lim = (ctypes.c_int * 4)(9, 9, 9, 9)
    assert lib.slam_pf_proposal_limits(lim) == 0 and list(lim) == [16, 0, 0, 0]
