"""FastSLAM 2.0 with unknown correspondences, the rule of include/ext/slamhip_proposal.h run literally in float64 on top of
oracle/pf_ref.py::OraclePF, and the scene the CPU and GPU tests of that rule share.

TEST INFRASTRUCTURE ONLY.  Every step of the header is one block below, in the header's order and with its names."""
import math

import numpy as np

from oracle import pf_ref as O

MAXOBS = 16


class ProposalUnknownPF(O.OraclePF):
    """OraclePF with ``step_proposal_unknown`` / ``associate_proposal``.

    pose_term=False leaves B B' out of the association's S (the FastSLAM-1.0 gate evaluated at the mean pose): only there to show
    that a test sees the term.  After a call: ``last_nis`` [m, n] the nis of the winning slot (NaN where nothing matched),
    ``last_capacity`` [m, n] True where a new landmark found no unused slot (reported as -2)."""

    pose_term = True

    def _mean(self, V, G, wheelbase, Q, dt):
        Q = np.asarray(Q, dtype=np.float64)
        x, y, phi = self.pose
        lq00 = math.sqrt(Q[0, 0])
        lq10 = 0.5 * (Q[0, 1] + Q[1, 0]) / lq00
        lq11 = math.sqrt(Q[1, 1] - lq10 * lq10)
        s, c = np.sin(G + phi), np.cos(G + phi)                       # oracle/pf_ref.py: step_proposal, term for term
        vts, vtc = V * dt * s, V * dt * c
        xm, ym = x + vtc, y + vts
        pm = O._wrap(phi + V * dt * math.sin(G) / wheelbase)
        gu20, gu21 = dt * math.sin(G) / wheelbase, V * dt * math.cos(G) / wheelbase
        gl = (dt * c * lq00 + (-vts) * lq10, (-vts) * lq11, dt * s * lq00 + vtc * lq10, vtc * lq11,
              gu20 * lq00 + gu21 * lq10, gu21 * lq11)
        return (lq00, lq10, lq11), (xm, ym, pm), gl

    # step 2 -------------------------------------------------------------------------------------------------------------------
    def _associate(self, mean, gl, z, R, gate1, gate2):
        xm, ym, pm = mean
        gl00, gl01, gl10, gl11, gl20, gl21 = gl
        m = z.shape[1]
        best_nd = np.full((m, self.n), np.inf)
        best_l = np.full((m, self.n), -1, dtype=np.int64)
        best_nis = np.full((m, self.n), np.nan)
        near = np.zeros((m, self.n), dtype=bool)
        for l in range(self.nl):
            lx, ly, pxx, pxy, pyy = self.lm[l]
            ok = pxx >= 0.0
            with np.errstate(all="ignore"):
                dx, dy = lx - xm, ly - ym
                d2 = dx * dx + dy * dy
                d = np.sqrt(d2)
                zp1 = np.arctan2(dy, dx) - pm
                h00, h01, h10, h11 = dx / d, dy / d, -dy / d2, dx / d2
                t00 = pxx * h00 + pxy * h01
                t01 = pxx * h10 + pxy * h11
                t10 = pxy * h00 + pyy * h01
                t11 = pxy * h10 + pyy * h11
                s00 = h00 * t00 + h01 * t10 + R[0, 0]
                s01 = h00 * t01 + h01 * t11 + R[0, 1]
                s10 = h10 * t00 + h11 * t10 + R[1, 0]
                s11 = h10 * t01 + h11 * t11 + R[1, 1]
                if self.pose_term:
                    b00 = -(h00 * gl00 + h01 * gl10)
                    b01 = -(h00 * gl01 + h01 * gl11)
                    b10 = -(h10 * gl00 + h11 * gl10) - gl20
                    b11 = -(h10 * gl01 + h11 * gl11) - gl21
                    s00 = s00 + (b00 * b00 + b01 * b01)
                    s01 = s01 + (b00 * b10 + b01 * b11)
                    s10 = s10 + (b10 * b00 + b11 * b01)
                    s11 = s11 + (b10 * b10 + b11 * b11)
                det = s00 * s11 - s01 * s10
                rdet = 1.0 / det
                qa, qb, qc = s11 * rdet, -(s01 + s10) * rdet, s00 * rdet
                logdet = np.log(det)
                for i in range(m):
                    v0 = z[0, i] - d
                    v1 = O._wrap(z[1, i] - zp1)
                    nis = qa * v0 * v0 + qb * v0 * v1 + qc * v1 * v1
                    nd = nis + logdet
                    better = ok & (nis < gate1) & (nd < best_nd[i])            # strict: the lowest slot wins a tie
                    best_nd[i] = np.where(better, nd, best_nd[i])
                    best_l[i] = np.where(better, l, best_l[i])
                    best_nis[i] = np.where(better, nis, best_nis[i])
                    near[i] |= ok & (nis <= gate2)
        self.last_nis = best_nis
        return np.where(best_l >= 0, best_l, np.where(near, -2, -1))

    def associate_proposal(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2):
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        R = np.asarray(R, dtype=np.float64)
        _, mean, gl = self._mean(V, G, wheelbase, Q, dt)
        return self._associate(mean, gl, z, R, gate1, gate2)

    def step_proposal_unknown(self, V, G, wheelbase, Q, dt, z, R, gate1, gate2):
        z = np.asarray(z, dtype=np.float64).reshape(2, -1)
        R = np.asarray(R, dtype=np.float64)
        m = z.shape[1]
        assert m <= MAXOBS
        (lq00, lq10, lq11), (xm, ym, pm), gl = self._mean(V, G, wheelbase, Q, dt)           # step 1
        gl00, gl01, gl10, gl11, gl20, gl21 = gl
        assoc = self._associate((xm, ym, pm), gl, z, R, gate1, gate2)                       # step 2
        # step 3: the proposal over the matched observations, every record read from the prior map
        prior = self.lm.copy()
        pidx = np.arange(self.n)
        mu0 = np.zeros(self.n)
        mu1 = np.zeros(self.n)
        g00 = np.ones(self.n)
        g01 = np.zeros(self.n)
        g11 = np.ones(self.n)
        logw = self.logw
        for i in range(m):
            hit = assoc[i] >= 0
            if not hit.any():
                continue
            slot = np.where(hit, assoc[i], 0)                          # a decision < 0 never becomes an index
            lx, ly, pxx, pxy, pyy = prior[slot, :, pidx].T
            r, b = z[0, i], z[1, i]
            with np.errstate(all="ignore"):
                dx, dy = lx - xm, ly - ym
                d2 = dx * dx + dy * dy
                d = np.sqrt(d2)
                h00, h01, h10, h11 = dx / d, dy / d, -dy / d2, dx / d2
                b00 = -(h00 * gl00 + h01 * gl10)
                b01 = -(h00 * gl01 + h01 * gl11)
                b10 = -(h10 * gl00 + h11 * gl10) - gl20
                b11 = -(h10 * gl01 + h11 * gl11) - gl21
                v0 = (r - d) - (b00 * mu0 + b01 * mu1)
                v1 = O._wrap(b - (np.arctan2(dy, dx) - pm)) - (b10 * mu0 + b11 * mu1)
                t00 = pxx * h00 + pxy * h01
                t01 = pxx * h10 + pxy * h11
                t10 = pxy * h00 + pyy * h01
                t11 = pxy * h10 + pyy * h11
                f00 = h00 * t00 + h01 * t10 + R[0, 0]
                f01 = 0.5 * ((h00 * t01 + h01 * t11 + R[0, 1]) + (h10 * t00 + h11 * t10 + R[1, 0]))
                f11 = h10 * t01 + h11 * t11 + R[1, 1]
                q00 = g00 * b00 + g01 * b01
                q01 = g00 * b10 + g01 * b11
                q10 = g01 * b00 + g11 * b01
                q11 = g01 * b10 + g11 * b11
                s00 = b00 * q00 + b01 * q10 + f00
                s01 = 0.5 * ((b00 * q01 + b01 * q11 + f01) + (b10 * q00 + b11 * q10 + f01))
                s11 = b10 * q01 + b11 * q11 + f11
                u00 = np.sqrt(s00)
                u01 = s01 / u00
                u11 = np.sqrt(s11 - u01 * u01)
                c00, c01, c11 = 1.0 / u00, -u01 / (u00 * u11), 1.0 / u11
                w00 = q00 * c00
                w01 = q00 * c01 + q01 * c11
                w10 = q10 * c00
                w11 = q10 * c01 + q11 * c11
                y0 = c00 * v0
                y1 = c01 * v0 + c11 * v1
                n_mu0 = mu0 + (w00 * y0 + w01 * y1)
                n_mu1 = mu1 + (w10 * y0 + w11 * y1)
                n_g00 = np.maximum(g00 - (w00 * w00 + w01 * w01), 0.0)                 # the guard: Sig stays positive semi-definite
                n_g01 = g01 - (w00 * w10 + w01 * w11)
                n_g11 = np.maximum(g11 - (w10 * w10 + w11 * w11), 0.0)
                gdet = n_g00 * n_g11
                n_g01 = np.where(n_g01 * n_g01 > gdet, np.copysign(np.sqrt(gdet), n_g01), n_g01)
                n_logw = logw - 0.5 * (y0 * y0 + y1 * y1) - np.log(u00 * u11) - math.log(2 * math.pi)
            mu0, mu1 = np.where(hit, n_mu0, mu0), np.where(hit, n_mu1, mu1)
            g00, g01, g11 = np.where(hit, n_g00, g00), np.where(hit, n_g01, g01), np.where(hit, n_g11, g11)
            logw = np.where(hit, n_logw, logw)
        # step 4: the draw
        x, y, phi = self.pose
        e1, e2 = O.normals2(self.gids, self.step, O.STREAM_PREDICT, self.seed)
        l00 = np.sqrt(g00)
        with np.errstate(all="ignore"):
            l10 = np.where(l00 > 0.0, g01 / l00, 0.0)
        l11 = np.sqrt(np.maximum(g11 - l10 * l10, 0.0))
        w0 = mu0 + l00 * e1
        w1 = mu1 + l10 * e1 + l11 * e2
        Vn = V + lq00 * w0
        Gn = G + (lq10 * w0 + lq11 * w1)
        self.pose = np.stack([x + Vn * dt * np.cos(Gn + phi), y + Vn * dt * np.sin(Gn + phi),
                              O._wrap(phi + Vn * dt * np.sin(Gn) / wheelbase)])
        self.step += 1
        # step 5: apply in observation order from the sampled pose (the bookkeeping of OraclePF.update_unknown), weight left alone
        saved_seen = self.seen.copy()
        capacity = np.zeros((m, self.n), dtype=bool)
        out = assoc.copy()
        for i in range(m):
            a = assoc[i].copy()
            newp = a == -1
            if newp.any():
                free = self.lm[:, 2, :] < 0.0
                first_free = np.argmax(free, axis=0)
                has_free = free[first_free, pidx]
                capacity[i] = newp & ~has_free
                a = np.where(newp, np.where(has_free, first_free, -2), a)
                out[i] = np.where(capacity[i], -2, out[i])
            for l in range(self.nl):
                sel = a == l
                for mask, seen_flag in ((sel & ~newp, True), (sel & newp, False)):
                    if not mask.any():
                        continue
                    sub = O.OraclePF.__new__(O.OraclePF)
                    sub.pose = self.pose[:, mask]
                    sub.lm = self.lm[:, :, mask].copy()
                    sub.logw = np.zeros(int(mask.sum()))
                    sub.seen = np.zeros(self.nl, dtype=bool)
                    sub.seen[l] = seen_flag
                    O.OraclePF.update_known(sub, z[:, i:i + 1], [l + 1], R)
                    self.lm[:, :, mask] = sub.lm
        self.seen = saved_seen
        self.logw = logw
        self.last_capacity = capacity
        return out


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
N, SLOTS, SEED = 1513, 8, 11
START = (0.5, -0.5, 0.3)
LANDMARKS = np.array([(12, 3), (6, -9), (-10, 4), (15, -2), (-4, -12), (9, 11), (-13, -6), (3, 14)], dtype=np.float64)
NINTH = np.array([7.0, 6.0])                                    # a ninth landmark for runs that must exhaust the 8 slots
V, DT, WHEELBASE = 3.0, 0.1, 4.0
Q = np.diag([0.5 ** 2, math.radians(3.0) ** 2])
R = np.diag([0.05 ** 2, math.radians(0.5) ** 2])
GATE1, GATE2 = 9.2, 25.0
STEPS = 12


def steer(t):
    return 0.05 * math.sin(0.7 * t)


def scene(steps=STEPS, ninth_from=None):
    """[(G_t, z_t)]: the truth driven with control noise from default_rng(77), observation noise from default_rng(5), four
    observations per step of the landmarks (t + k) mod 8, k = 0..3.  ``ninth_from``: from that step on a fifth observation, of
    NINTH, is appended (noise from default_rng(9), so that the first four stay what they are)."""
    ctl, obs, extra = np.random.default_rng(77), np.random.default_rng(5), np.random.default_rng(9)
    x, y, phi = START
    out = []
    for t in range(steps):
        G = steer(t)
        Vn = V + math.sqrt(Q[0, 0]) * ctl.standard_normal()            # (slam.jl_amd/sim.py: speed, then steering)
        Gn = G + math.sqrt(Q[1, 1]) * ctl.standard_normal()
        x, y, phi = (x + Vn * DT * math.cos(Gn + phi), y + Vn * DT * math.sin(Gn + phi),
                     float(O._wrap(phi + Vn * DT * math.sin(Gn) / WHEELBASE)))
        ids = [(t + k) % 8 for k in range(4)]
        lms = [LANDMARKS[j] for j in ids]
        if ninth_from is not None and t >= ninth_from:
            lms.append(NINTH)
        z = np.zeros((2, len(lms)))
        for i, lm in enumerate(lms):
            dx, dy = lm[0] - x, lm[1] - y
            z[0, i] = math.hypot(dx, dy)
            z[1, i] = float(O._wrap(math.atan2(dy, dx) - phi))
        # the noise as slam.jl_amd/sim.py::get_observations draws it: the step's ranges first, then its bearings
        z[:, :4] += np.vstack([obs.standard_normal(4) * math.sqrt(R[0, 0]), obs.standard_normal(4) * math.sqrt(R[1, 1])])
        if len(lms) > 4:
            z[:, 4] += extra.standard_normal(2) * np.sqrt(np.diag(R))
        out.append((G, z))
    return out


def fresh(cls=ProposalUnknownPF, n=N, slots=SLOTS, seed=SEED):
    pf = cls(n, slots, seed)
    pf.set_pose(START)
    pf.clear_landmarks()
    return pf


def run(rule, steps=None, q=Q, gate_scale=1.0, pose_term=True, n=N):
    """The scene through ``rule`` ("2.0": step_proposal_unknown; "1.0": predict + update_unknown), normalised every step, no
    resampling.  Returns (decisions per step, Neff / n per step, the filter)."""
    pf = fresh(n=n)
    pf.pose_term = pose_term
    decisions, neff = [], []
    for G, z in (steps if steps is not None else scene()):
        if rule == "2.0":
            a = pf.step_proposal_unknown(V, G, WHEELBASE, q, DT, z, R, GATE1 * gate_scale, GATE2 * gate_scale)
        else:
            pf.predict(V, G, WHEELBASE, q, DT)
            a = pf.update_unknown(z, R, GATE1 * gate_scale, GATE2 * gate_scale)
        gm, s1, s2 = pf.weight_stats()
        pf.normalize(gm, s1)
        decisions.append(np.array(a))
        neff.append(s1 * s1 / s2 / pf.n)
    return decisions, neff, pf


def counts(decisions):
    a = np.concatenate([d.reshape(-1) for d in decisions])
    return int((a >= 0).sum()), int((a == -1).sum()), int((a == -2).sum())
