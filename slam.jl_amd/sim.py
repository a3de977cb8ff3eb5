"""Headless, seeded, sleep-free driver with the call pattern of the reference's
``sim!`` (sim/ekfslam-sim.jl:54-143).  SURVEY.md section 8(f) row N1.

This is HOST logic around the hot path, not the hot path: vehicle kinematics,
the waypoint follower and the simulated sensor are a few scalar operations per
step and stay on the CPU exactly as in the reference.  The filter is an object
passed in by the caller with the reference's four entry points

    filt.predict(v, g, wheelbase, Q, dt)
    zf, idf, zn = filt.associate(z, R, gate1, gate2)
    filt.update(zf, R, idf)
    filt.add_features(zn, R)
    filt.pose() -> (x, y, phi)

(``slam.jl_amd.ekf.EKFSlamState`` provides them on the GPU; the tests wrap the
oracle the same way).  Nothing here imports the oracle.

Differences from the reference, all deliberate and test-visible:
* the real-time frame limiter ``sleep`` (sim/ekfslam-sim.jl:132-136) and the
  pause loop (:138-140) are dropped -- they are UI pacing, not work;
* the unseeded global RNG (sim/sim-utils.jl:5,36-37,68) is replaced by a
  seeded ``numpy.random.Generator``; draw order follows the reference:
  speed noise, steering noise per step; then per observation step one row of
  range draws followed by one row of bearing draws;
* every filter input is recorded (``SimLog``) so a run can be replayed through
  another filter without the RNG.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np


def mpi_to_pi(phi: float) -> float:
    """Single conditional wrap, src/common.jl:102-110."""
    if phi > math.pi:
        return phi - 2 * math.pi
    if phi < -math.pi:
        return phi + 2 * math.pi
    return phi


def get_waypoints(txtfile) -> np.ndarray:
    """2 x N waypoint array from a header + 2-column text file (src/common.jl:84-87)."""
    return np.loadtxt(txtfile, skiprows=1).T


def make_landmarks(n: int, boundaries, margin: float, rng: np.random.Generator) -> np.ndarray:
    """sim/sim-utils.jl:1-6 -- every coordinate drawn uniformly from the pool
    ``[xmin+bx : xmax-bx ; ymin+by : ymax-by]`` (unit-step ranges, so whole
    numbers for the reference's 0..100 scene)."""
    xmin, xmax, ymin, ymax = boundaries
    bx = margin * (xmax - xmin)
    by = margin * (ymax - ymin)
    pool = np.concatenate([np.arange(xmin + bx, xmax - bx + 1e-9, 1.0),
                           np.arange(ymin + by, ymax - by + 1e-9, 1.0)])
    return pool[rng.integers(0, len(pool), size=(2, n))]


@dataclass
class Vehicle:
    """The fields of src/common.jl:36-57 that the filter path touches."""
    wheelbase: float = 4.0                      # sim/ekfslam-sim.jl:30
    max_gamma: float = 60 * math.pi / 180       # :31
    steer_rate: float = 60 * math.pi / 180      # :32
    sensor_range: float = 30.0                  # :33
    pose: np.ndarray = field(default_factory=lambda: np.zeros(3))
    target_speed: float = 8.0                   # :36
    measured_speed: float = 0.0
    target_gamma: float = 0.0
    measured_gamma: float = 0.0
    waypoint_id: int = 1                        # 1-based, 0 = finished


def initial_pose(waypoints: np.ndarray) -> np.ndarray:
    """src/common.jl:93-96."""
    return np.array([waypoints[0, 0], waypoints[1, 0],
                     math.atan2(waypoints[1, 1] - waypoints[1, 0],
                                waypoints[0, 1] - waypoints[0, 0])])


def step_vehicle(vehicle: Vehicle, dt: float) -> None:
    """src/common.jl:172-181 (ideal speed / steering angle)."""
    x, y, phi = vehicle.pose
    v, g = vehicle.target_speed, vehicle.target_gamma
    vehicle.pose = np.array([x + v * dt * math.cos(g + phi),
                             y + v * dt * math.sin(g + phi),
                             mpi_to_pi(phi + v * dt * math.sin(g) / vehicle.wheelbase)])


def steer(vehicle: Vehicle, waypoints: np.ndarray, d_min: float, dt: float) -> None:
    """src/common.jl:189-230."""
    g = vehicle.target_gamma
    iwp = vehicle.waypoint_id
    x, y, phi = vehicle.pose
    cwp = waypoints[:, iwp - 1]
    d2 = (cwp[0] - x) ** 2 + (cwp[1] - y) ** 2
    if d2 < d_min ** 2:
        iwp += 1
        if iwp > waypoints.shape[1]:
            vehicle.waypoint_id = 0
            return
        cwp = waypoints[:, iwp - 1]
    dg = mpi_to_pi(math.atan2(cwp[1] - y, cwp[0] - x) - phi - g)
    dgmax = vehicle.steer_rate * dt
    if abs(dg) > dgmax:
        dg = math.copysign(dgmax, dg)
    g += dg
    if abs(g) > vehicle.max_gamma:
        g = math.copysign(vehicle.max_gamma, g)
    vehicle.target_gamma = g
    vehicle.waypoint_id = iwp


def get_observations(vehicle: Vehicle, landmarks: np.ndarray, R, rng):
    """sim/sim-utils.jl:12-28,53-75.  Returns (z 2 x nz, tags 1-based)."""
    x, y, phi = vehicle.pose
    dx = landmarks[0] - x
    dy = landmarks[1] - y
    near = [i for i in range(landmarks.shape[1])
            if (dx[i] * math.cos(phi) + dy[i] * math.sin(phi)) > 0
            and (dx[i] ** 2 + dy[i] ** 2) < vehicle.sensor_range ** 2]
    near = np.asarray(near, dtype=np.int64)
    z = np.vstack([np.sqrt(dx[near] ** 2 + dy[near] ** 2),
                   np.arctan2(dy[near], dx[near]) - phi])
    if z.shape[1] > 0:
        z = z + np.vstack([rng.standard_normal(z.shape[1]) * math.sqrt(R[0, 0]),
                           rng.standard_normal(z.shape[1]) * math.sqrt(R[1, 1])])
    return z, near + 1


@dataclass
class SimLog:
    """Everything the filter was fed, in call order, plus both tracks."""
    controls: list = field(default_factory=list)        # (v, g) per predict
    obs_steps: list = field(default_factory=list)       # predict-step index of each observation step
    observations: list = field(default_factory=list)    # z (2 x nz) per observation step
    assoc: list = field(default_factory=list)           # (idf list, n_new) per observation step
    pruned: list = field(default_factory=list)          # (observation step, removed ids) per removal (sim(prune_after=k))
    merged: list = field(default_factory=list)          # (observation step, pairs) per merge (sim(merge_gate=g))
    joined: list = field(default_factory=list)          # (observation step, first_new, landmarks joined, landmarks after) per join (sim(submap_steps=k))
    true_track: list = field(default_factory=list)
    slam_track: list = field(default_factory=list)
    nees: list = field(default_factory=list)            # (predict-step index, NEES, degrees of freedom 3 + 2 N) per sim(nees_every=k) sample
    nees_truth: list = field(default_factory=list)      # the true state each sample was held against (pose, then the map's landmarks)
    landmark_tags: object = None                        # sim(nees_every=k): 1-based true landmark behind each map landmark at the end
    best_path: object = None                            # [L, 3]: the best particle's path at the end of the run (a PFSlamState after track_path)
    fixes: list = field(default_factory=list)           # (predict-step index, measured xy) per position fix (sim(fix_every=k))
    areas: list = field(default_factory=list)           # (observation step, local landmarks, landmarks added, N after) per closed local area (sim(local_radius=r))


#: constants of sim/ekfslam-sim.jl:62-76,114
SIGMA_SPEED = 0.5
SIGMA_STEER = 3.0 * math.pi / 180
SIGMA_R = 0.1
SIGMA_B = 1.0 * math.pi / 180
DT = 0.025
DT_OBS = 8 * DT
GATE1 = 4.0
GATE2 = 25.0
D_MIN = 1.0


def default_QR():
    Q = np.array([[SIGMA_SPEED ** 2, 0.0], [0.0, SIGMA_STEER ** 2]])
    R = np.array([[SIGMA_R ** 2, 0.0], [0.0, SIGMA_B ** 2]])
    return Q, R


def sim(filt, waypoints: np.ndarray, landmarks: np.ndarray, seed: int, nlaps: int = 2,
        max_steps: int = 100000, monitor=None, fused: bool = False, prune_after=None, merge_gate=None,
        submap_steps=None, association: str = "nearest", nees_every=None, fix_every: int = 0,
        fix_sigma: float = 0.5, local_radius=None, iterated=None, fej: bool = False, fej_joint: bool = False) -> SimLog:
    """The loop of sim/ekfslam-sim.jl:80-141 without sleep/pause.

    ``filt`` must already hold the initial state (x = initial pose, P = 0).
    ``fused``: use ``filt.observe`` (associate + update + add_features in one library call,
    same results) instead of the three calls of :114-120.
    ``prune_after``: None (default) is the reference's loop, whose map only grows.  An integer k (no counterpart in the
    reference): a landmark that has been matched only by the observation that created it and is not matched in the k
    observation steps after its creation is removed with ``filt.remove_landmarks(ids) -> new_index``.  The per-landmark
    counters live here on the host (the association comes back to the host anyway) and are renumbered through
    ``new_index``; removals are recorded in ``log.pruned`` with the ids they had at that moment.
    ``merge_gate``: None (default) changes nothing.  A number g (no counterpart in the reference): after every observation
    step ``filt.find_duplicates(g) -> (pairs, count)`` looks for landmarks entered twice and ``filt.merge_landmarks(pairs) ->
    new_index`` fuses them; the ``prune_after`` counters follow ``new_index`` (a merged landmark keeps the earlier birth and
    the larger match count).  Merges are recorded in ``log.merged``.
    ``submap_steps``: None (default) is the loop above.  An integer k (map joining, no counterpart in the reference): ``filt`` is
    the GLOBAL map and stays frozen while a local map ``filt.submap(filt.max_landmarks)`` -- pose 0, P = 0, its frame the global
    vehicle pose -- takes every predict and observation; after k observation steps (and once more when the course ends) it is
    joined with ``filt.join(local, merge_gate=merge_gate)``, closed, and a new one starts.  With ``merge_gate`` the join fuses the
    landmarks both maps hold (there is no per-step merge in this mode; ``prune_after`` is refused).  Joins are recorded in
    ``log.joined``; ``log.slam_track`` holds the local pose composed with the frozen global one.
    ``association``: "nearest" (default) is the reference's nearest neighbour.  "joint" (no counterpart in the reference) takes
    the decisions from the joint-compatibility search, ``filt.associate_joint`` / ``filt.observe_joint`` with their defaults: no
    landmark is used twice in one step (at most 64 observations per step; not available with ``submap_steps``).
    ``nees_every``: None (default) changes nothing.  An integer k (no counterpart in the reference): after every k-th step the
    consistency measure ``filt.nees(x_true)`` -- e' P^-1 e over the vehicle and every landmark seen so far, from the factor of P
    on the device -- is recorded in ``log.nees`` with its degrees of freedom, and ``x_true`` in ``log.nees_truth``.  ``x_true`` is the
    simulator's vehicle pose and, for each landmark of the map, the TRUE correspondence: the simulator's landmark whose observation
    created it (the sensor's tags, which the filter never sees, are carried here through every new feature, removal and merge; a
    merged landmark keeps the tag of its lowest old id).  A wrong association therefore counts against the filter, as it should.
    A matrix that has no Cholesky factor is recorded as NaN.  Not available with ``submap_steps`` (the truth is in another frame there).
    ``fix_every``: 0 (default) changes nothing.  An integer k (no counterpart in the reference): at the end of every k-th step a
    position fix -- the true position plus noise of standard deviation ``fix_sigma`` per axis, a GPS receiver -- is applied with
    ``filt.fix_position(xy, fix_sigma^2 I)``.  Its noise comes from a generator of its own (seeded from ``seed``), so every other
    draw of the run is what it is without fixes.  Fixes are recorded in ``log.fixes``.  Not available with ``submap_steps``.
    ``local_radius``: None (default) changes nothing.  A number r (the compressed EKF, no counterpart in the reference): every
    predict and observation goes to a local area ``filt.local(filt.landmarks_within(cx, cy, r))`` around the pose (cx, cy) at which
    it was opened, and ``filt`` itself is brought up to date only when the area is closed: before an observation step at which the
    vehicle is nearer to the rim than the sensor range plus a margin of LOCAL_MARGIN = 2 m (|pose - centre| + sensor_range + 2 > r:
    the margin covers the pose error and the landmarks' own, so that nothing the sensor can see lies outside the area), and once
    more when the course ends.  r must exceed sensor_range + 2.  Up to rounding the run is the plain loop's; ``log.assoc`` holds
    GLOBAL ids.  Closed areas are recorded in ``log.areas``.  Only with the plain loop's other options at their defaults.
    ``iterated``: None (default) changes nothing.  An integer k (the iterated EKF, no counterpart in the reference): the update of
    every observation step is ``filt.update_iterated(zf, R, idf, max_iter=k)`` -- relinearised up to k times, more than 8 matched
    observations in consecutive batches of 8 -- after the nearest-neighbour association; with ``fused`` the three calls are
    ``filt.observe_iterated``.  Not available with joint association, ``submap_steps`` or ``local_radius``.
    ``fej``: False (default) changes nothing.  True (first-estimates Jacobians, no counterpart in the reference): predict, update and
    add_features go through ``filt.fej()`` -- the Jacobians evaluated at every landmark's first estimate and at the predicted pose,
    the association at the current estimates as before; with ``fused`` the observation step is that object's ``observe`` (joint
    association: the three calls, fused or not).  Not available with ``submap_steps``, ``local_radius``, ``iterated``, ``prune_after`` or ``merge_gate``.
    ``fej_joint``: False (default) changes nothing.  True, only with ``fej``: the step's update is that object's ``update_joint`` --
    all matched observations of the step in one update (consecutive batches of 64) -- where ``update`` chains batches of 8.
    """
    if fej_joint and not fej:
        raise ValueError("fej_joint needs fej=True")
    if fej and (submap_steps is not None or local_radius is not None or iterated is not None or prune_after is not None
                or merge_gate is not None):
        raise ValueError("fej is not available with submap_steps, local_radius, iterated, prune_after or merge_gate")
    if iterated is not None:
        iterated = int(iterated)
        if iterated < 1 or association != "nearest" or submap_steps is not None or local_radius is not None:
            raise ValueError("iterated must be a positive iteration count and is not available with joint association, "
                             "submap_steps or local_radius")
    if local_radius is not None:
        if (prune_after is not None or merge_gate is not None or submap_steps is not None or association != "nearest"
                or nees_every is not None or fix_every):
            raise ValueError("local_radius is not available together with prune_after, merge_gate, submap_steps, joint "
                             "association, nees_every or fix_every")
        return _sim_local(filt, waypoints, landmarks, seed, nlaps, max_steps, monitor, fused, float(local_radius))
    fix_every = int(fix_every)
    if fix_every < 0 or (fix_every and submap_steps is not None):
        raise ValueError("fix_every must be a non-negative step count and is not available with submap_steps")
    if association not in ("nearest", "joint"):
        raise ValueError('association must be "nearest" or "joint"')
    joint = association == "joint"
    if joint and submap_steps is not None:
        raise ValueError('association="joint" is not available with submap_steps')
    if nees_every is not None and (submap_steps is not None or int(nees_every) < 1):
        raise ValueError("nees_every must be a positive step count and is not available with submap_steps")
    if submap_steps is not None:
        if prune_after is not None:
            raise ValueError("prune_after counts matches in one map: not available with submap_steps")
        return _sim_submaps(filt, waypoints, landmarks, seed, nlaps, max_steps, monitor, fused, merge_gate, int(submap_steps))
    rng = np.random.default_rng(seed)
    fix_rng = np.random.default_rng([int(seed), 0x6669]) if fix_every else None
    Q, R = default_QR()
    vehicle = Vehicle(pose=initial_pose(waypoints))
    log = SimLog()
    dtsum = 0.0
    nsteps = 0
    born = np.zeros(0, dtype=np.int64)      # prune_after: observation step that created landmark j (at [j - 1]) ...
    hits = np.zeros(0, dtype=np.int64)      # ... and its matches since
    tags = np.zeros(0, dtype=np.int64)      # nees_every: the true landmark (1-based) whose observation created landmark j
    step = filt.fej() if fej else filt      # what takes predict / update / add_features / observe; everything else goes to filt
    while vehicle.waypoint_id != 0 and nsteps < max_steps:
        steer(vehicle, waypoints, D_MIN, DT)                              # :85
        if vehicle.waypoint_id == 0 and nlaps > 1:                        # :88-91
            vehicle.waypoint_id = 1
            nlaps -= 1
        step_vehicle(vehicle, DT)                                         # :94
        vehicle.measured_speed = vehicle.target_speed + rng.standard_normal() * math.sqrt(Q[0, 0])
        vehicle.measured_gamma = vehicle.target_gamma + rng.standard_normal() * math.sqrt(Q[1, 1])
        step.predict(vehicle.measured_speed, vehicle.measured_gamma, vehicle.wheelbase, Q, DT)  # :100
        log.controls.append((vehicle.measured_speed, vehicle.measured_gamma))
        dtsum += DT                                                       # :102
        if dtsum > DT_OBS:                                                # :105 (fires every 9th step)
            dtsum = 0.0
            z, ztags = get_observations(vehicle, landmarks, R, rng)       # :108
            if fused and not (fej and joint):
                if iterated is not None:
                    assoc = np.asarray(filt.observe_iterated(z, R, GATE1, GATE2, max_iter=iterated)[0])
                else:
                    assoc = np.asarray(filt.observe_joint(z, R, GATE1, GATE2)[0] if joint else
                                       (step.observe(z, R, GATE1, GATE2, joint=True) if fej_joint else step.observe(z, R, GATE1, GATE2)))   # :114-120 in one call
                idf = assoc[assoc > 0]
                zn = np.asarray(z, dtype=float).reshape(2, -1)[:, assoc < 0]
            else:
                zf, idf, zn = filt.associate_joint(z, R, GATE1, GATE2)[:3] if joint else filt.associate(z, R, GATE1, GATE2)   # :114
                if iterated is not None:
                    filt.update_iterated(zf, R, idf, max_iter=iterated)
                else:
                    (step.update_joint if fej_joint else step.update)(zf, R, idf)     # :117
                step.add_features(zn, R)                                  # :120
            log.obs_steps.append(nsteps)
            log.observations.append(np.array(z))
            log.assoc.append((np.asarray(idf).reshape(-1).tolist(), int(np.asarray(zn).reshape(2, -1).shape[1])))
            if nees_every is not None:
                tags = np.concatenate([tags, ztags[_columns_of(z, zn)]])
            if prune_after is not None:
                t = len(log.obs_steps) - 1
                np.add.at(hits, np.asarray(idf, dtype=np.int64).reshape(-1) - 1, 1)
                nn = log.assoc[-1][1]
                born = np.concatenate([born, np.full(nn, t, dtype=np.int64)])
                hits = np.concatenate([hits, np.zeros(nn, dtype=np.int64)])
                stale = np.flatnonzero((hits == 0) & (t - born >= int(prune_after)))
                if stale.size:
                    new_index = np.asarray(filt.remove_landmarks(stale + 1))
                    log.pruned.append((t, (stale + 1).tolist()))
                    left = new_index > 0
                    born, hits = born[left], hits[left]
                    if nees_every is not None:
                        tags = tags[left]
            if merge_gate is not None:
                pairs, _count = filt.find_duplicates(merge_gate)
                if len(pairs):
                    new_index = np.asarray(filt.merge_landmarks(pairs), dtype=np.int64)
                    log.merged.append((len(log.obs_steps) - 1, np.asarray(pairs).tolist()))
                    if nees_every is not None:
                        stays = np.flatnonzero(new_index > 0)[::-1]       # (the lowest old id of a merged group is written last)
                        ntags = np.zeros(int(new_index.max()) if new_index.size else 0, dtype=np.int64)
                        ntags[new_index[stays] - 1] = tags[stays]
                        tags = ntags
                    if prune_after is not None:
                        nleft = int(new_index.max()) if new_index.size else 0
                        nborn = np.full(nleft, np.iinfo(np.int64).max, dtype=np.int64)
                        nhits = np.zeros(nleft, dtype=np.int64)
                        np.minimum.at(nborn, new_index - 1, born)
                        np.maximum.at(nhits, new_index - 1, hits)
                        born, hits = nborn, nhits
        nsteps += 1
        if fix_every and nsteps % fix_every == 0:
            xy = np.asarray(vehicle.pose[:2], dtype=float) + fix_rng.standard_normal(2) * float(fix_sigma)
            filt.fix_position(xy, np.eye(2) * float(fix_sigma) ** 2)
            log.fixes.append((nsteps, xy))
        log.true_track.append(np.array(vehicle.pose))
        log.slam_track.append(np.array(filt.pose()))
        if nees_every is not None and nsteps % int(nees_every) == 0:
            value, x_true = _nees_against_truth(filt, vehicle, landmarks, tags)
            log.nees.append((nsteps, value, int(x_true.size)))
            log.nees_truth.append(x_true)
        if monitor is not None:
            monitor(vehicle, filt, nsteps)
    if fej:
        step.close()
    if nees_every is not None:
        log.landmark_tags = tags
    if getattr(filt, "path_history", None) is not None:                   # a PFSlamState that tracks its path (FastSLAM.track_path)
        log.best_path = np.array(filt.path())
    return log


LOCAL_MARGIN = 2.0


def _sim_local(filt, waypoints, landmarks, seed, nlaps, max_steps, monitor, fused, radius) -> SimLog:
    """sim(..., local_radius=r): the same vehicle, sensor and draw order as the plain loop; the filter calls go to a local area."""
    rng = np.random.default_rng(seed)
    Q, R = default_QR()
    vehicle = Vehicle(pose=initial_pose(waypoints))
    if not radius > vehicle.sensor_range + LOCAL_MARGIN:
        raise ValueError("local_radius must exceed the sensor range plus LOCAL_MARGIN")
    log = SimLog()
    dtsum = 0.0
    nsteps = 0

    def open_area():
        c = np.asarray(filt.pose(), dtype=float)[:2]
        return filt.local(filt.landmarks_within(c[0], c[1], radius)), c

    def close_area(area):
        gids = area.global_ids()
        added = int(area.info()["added"])
        area.close()
        log.areas.append((len(log.obs_steps) - 1, int(gids.size), added, int(filt.N)))
        area.destroy()

    area, centre = open_area()
    try:
        while vehicle.waypoint_id != 0 and nsteps < max_steps:
            steer(vehicle, waypoints, D_MIN, DT)
            if vehicle.waypoint_id == 0 and nlaps > 1:
                vehicle.waypoint_id = 1
                nlaps -= 1
            step_vehicle(vehicle, DT)
            vehicle.measured_speed = vehicle.target_speed + rng.standard_normal() * math.sqrt(Q[0, 0])
            vehicle.measured_gamma = vehicle.target_gamma + rng.standard_normal() * math.sqrt(Q[1, 1])
            area.predict(vehicle.measured_speed, vehicle.measured_gamma, vehicle.wheelbase, Q, DT)
            log.controls.append((vehicle.measured_speed, vehicle.measured_gamma))
            dtsum += DT
            if dtsum > DT_OBS:
                dtsum = 0.0
                z, _tags = get_observations(vehicle, landmarks, R, rng)
                pose = np.asarray(area.state.pose(), dtype=float)
                if math.hypot(pose[0] - centre[0], pose[1] - centre[1]) + vehicle.sensor_range + LOCAL_MARGIN > radius:
                    close_area(area)
                    area, centre = open_area()
                if fused:
                    assoc = np.asarray(area.observe(z, R, GATE1, GATE2))
                    idf = assoc[assoc > 0]
                    zn = np.asarray(z, dtype=float).reshape(2, -1)[:, assoc < 0]
                else:
                    zf, idf, zn = area.associate(z, R, GATE1, GATE2)
                    area.update(zf, R, idf)
                    area.add_features(zn, R)
                gids = np.asarray(area.global_ids(), dtype=np.int64)
                log.obs_steps.append(nsteps)
                log.observations.append(np.array(z))
                log.assoc.append((gids[np.asarray(idf, dtype=np.int64).reshape(-1) - 1].tolist(),
                                  int(np.asarray(zn).reshape(2, -1).shape[1])))
            nsteps += 1
            log.true_track.append(np.array(vehicle.pose))
            log.slam_track.append(np.array(area.state.pose()))
            if monitor is not None:
                monitor(vehicle, filt, nsteps)
        close_area(area)
        area = None
    finally:
        if area is not None:
            area.destroy()
    return log


def _columns_of(z, zn):
    """The columns of z (2 x nz) that zn (2 x nn) was taken from, in zn's order: the filter hands new-feature observations back as
    they came, so they are found by value."""
    z = np.asarray(z, dtype=float).reshape(2, -1)
    zn = np.asarray(zn, dtype=float).reshape(2, -1)
    cols = np.zeros(zn.shape[1], dtype=np.int64)
    for k in range(zn.shape[1]):
        hit = np.flatnonzero((z[0] == zn[0, k]) & (z[1] == zn[1, k]))
        if hit.size != 1:
            raise RuntimeError("a new-feature observation is not one of the step's observations")
        cols[k] = hit[0]
    return cols


def _nees_against_truth(filt, vehicle, landmarks, tags):
    """(NEES, x_true) of ``filt`` against the simulator's truth: the vehicle pose and, per map landmark, the true landmark
    ``tags`` names (1-based).  NaN for a matrix without a Cholesky factor."""
    from ._lib import NotPositiveDefinite
    truth = np.asarray(landmarks, dtype=float).reshape(2, -1)
    if 3 + 2 * tags.size != filt.n:
        raise RuntimeError("the tags do not follow the map")
    x_true = np.concatenate([np.asarray(vehicle.pose, dtype=float), truth[:, tags - 1].T.reshape(-1)])
    try:
        return float(filt.nees(x_true)), x_true
    except NotPositiveDefinite:
        return float("nan"), x_true


def _compose(base, local):
    """The local pose in the frame of ``base``."""
    c, s_ = math.cos(base[2]), math.sin(base[2])
    return np.array([base[0] + c * local[0] - s_ * local[1], base[1] + s_ * local[0] + c * local[1],
                     mpi_to_pi(base[2] + local[2])])


def _sim_submaps(glob, waypoints, landmarks, seed, nlaps, max_steps, monitor, fused, merge_gate, k) -> SimLog:
    """sim(..., submap_steps=k): the same vehicle, sensor and draw order as the plain loop; the filter calls go to a local map."""
    if k < 1:
        raise ValueError("submap_steps must be at least 1")
    rng = np.random.default_rng(seed)
    Q, R = default_QR()
    vehicle = Vehicle(pose=initial_pose(waypoints))
    log = SimLog()
    dtsum = 0.0
    nsteps = 0
    base = np.array(glob.pose(), dtype=float)
    local = glob.submap(glob.max_landmarks)
    in_local = 0

    def close_local():
        nonlocal local, base, in_local
        nb = int(local.N)
        out = glob.join(local, merge_gate=merge_gate)
        first = int(out[0]) if merge_gate is not None else int(out)
        local.close()
        log.joined.append((len(log.obs_steps) - 1, first, nb, int(glob.N)))
        base = np.array(glob.pose(), dtype=float)
        in_local = 0

    try:
        while vehicle.waypoint_id != 0 and nsteps < max_steps:
            steer(vehicle, waypoints, D_MIN, DT)
            if vehicle.waypoint_id == 0 and nlaps > 1:
                vehicle.waypoint_id = 1
                nlaps -= 1
            step_vehicle(vehicle, DT)
            vehicle.measured_speed = vehicle.target_speed + rng.standard_normal() * math.sqrt(Q[0, 0])
            vehicle.measured_gamma = vehicle.target_gamma + rng.standard_normal() * math.sqrt(Q[1, 1])
            local.predict(vehicle.measured_speed, vehicle.measured_gamma, vehicle.wheelbase, Q, DT)
            log.controls.append((vehicle.measured_speed, vehicle.measured_gamma))
            dtsum += DT
            if dtsum > DT_OBS:
                dtsum = 0.0
                z, _tags = get_observations(vehicle, landmarks, R, rng)
                if fused:
                    assoc = np.asarray(local.observe(z, R, GATE1, GATE2))
                    idf = assoc[assoc > 0]
                    zn = np.asarray(z, dtype=float).reshape(2, -1)[:, assoc < 0]
                else:
                    zf, idf, zn = local.associate(z, R, GATE1, GATE2)
                    local.update(zf, R, idf)
                    local.add_features(zn, R)
                log.obs_steps.append(nsteps)
                log.observations.append(np.array(z))
                log.assoc.append((np.asarray(idf).reshape(-1).tolist(), int(np.asarray(zn).reshape(2, -1).shape[1])))
                in_local += 1
                if in_local == k:
                    close_local()
                    local = glob.submap(glob.max_landmarks)
            nsteps += 1
            log.true_track.append(np.array(vehicle.pose))
            log.slam_track.append(_compose(base, np.asarray(local.pose(), dtype=float)))
            if monitor is not None:
                monitor(vehicle, glob, nsteps)
        close_local()                                                     # what the last local map holds, the pose included
    finally:
        local.close()
    return log
