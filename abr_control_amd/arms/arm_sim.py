"""Rigid-body plant of ANY arm with the reference's ArmSim interface (abr_control/arms/twojoint/arm_sim.py:20-87):
connect / disconnect / reset / get_feedback / send_forces, for one arm (q of shape (n,)) or B arms (q_init of shape
(B, n)), stepped on the GPU by engine.plant_step: ddq = M^-1 (u - C dq - g) with the robot_config's own M, C and g, then
dq += ddq h, q += dq h, `substeps` times per call with h = dt / substeps (arms/threejoint/arm_sim.py:93-94 takes
dt / 1e-5 such substeps).  `effects` (_abi.make_plant_effects) makes the plant non-ideal: torque saturation, viscous and
smoothed Coulomb joint friction, hard joint limits with restitution; send_forces also takes a joint-space disturbance
`tau_ext` and a world-frame wrench at the end effector (include/abrk.h, abrk_plant_effects).  `payload` is a point mass
carried at the end effector - (m, r) for every arm, or [B, 4] rows of m, rx, ry, rz - which changes M, C and g of the
plant and which the robot_config (the controller's model) knows nothing of.  `surfaces` are planes the arm can touch: a
contact.ContactSurfaces, or planes [S, 8] / [B, S, 8] of nx, ny, nz, d, k, c, mu, rho for a tip at the origin of the
end-effector frame; the contact torque of the state at the start of a step is added to that step's tau_ext.
`obstacles` are spheres the whole arm can hit: a link_contact.Obstacles, or spheres [K, 7] / [B, K, 7] of cx, cy, cz, R,
k, c, mu for link capsules of the default radius; their torque is added to tau_ext too, after that of `surfaces`."""
import numpy as np

from .. import _abi, contact, engine, link_contact, plant_payload


class ArmSim:
    def __init__(self, robot_config, dt=0.001, q_init=None, substeps=1, gravity=True, effects=None, payload=None,
                 surfaces=None, obstacles=None):
        self.robot_config = robot_config
        n = robot_config.N_JOINTS
        q0 = q_init if q_init is not None else getattr(robot_config, "START_ANGLES", None)
        self.q_init = np.zeros(n) if q0 is None else np.array(q0, dtype=float)
        if self.q_init.ndim not in (1, 2) or self.q_init.shape[-1] != n:
            raise ValueError(f"q_init has shape {self.q_init.shape}; expected ({n},) or (B, {n})")
        self.dt = dt
        self.substeps = int(substeps)
        self.gravity = bool(gravity)
        self.effects = effects
        self.payload = self._payload_rows(payload)
        self.surfaces = surfaces
        self._contact_report = None
        self.obstacles = obstacles
        self._link_contact_report = None
        self.t = 0.0
        self.reset()

    @staticmethod
    def _payload_rows(payload):
        """None, (m, r) with r of three values, or [B, 4] / (4,) of m, rx, ry, rz -> None or a float array [.., 4]"""
        if payload is None:
            return None
        if isinstance(payload, tuple) and len(payload) == 2 and np.ndim(payload[0]) == 0:
            m, r = payload
            r = np.asarray(r, dtype=float)
            if r.shape != (3,):
                raise ValueError(f"payload offset has shape {r.shape}; expected (3,)")
            return np.concatenate([[float(m)], r])
        p = np.asarray(payload, dtype=float)
        if p.ndim not in (1, 2) or p.shape[-1] != 4:
            raise ValueError(f"payload has shape {p.shape}; expected (m, r), (4,) or (B, 4)")
        return p

    def set_payload(self, payload):
        """the payload carried from the next step on: None, (m, r), (4,) or (B, 4) of m, rx, ry, rz"""
        self.payload = self._payload_rows(payload)

    def _contact(self, q, dq, dtype):
        """-> the contact torque [B, n] of the state (q, dq) on self.surfaces; keeps the report"""
        rc, B = self.robot_config, q.shape[0]
        sf = self.surfaces
        if isinstance(sf, contact.ContactSurfaces):
            planes, params = contact.planes_rows(sf.planes, B), sf.params()
        else:
            planes = contact.planes_rows(sf, B)
            params = _abi.make_contact_params(rc.N_JOINTS, n_surfaces=planes.shape[1])
        tau, self._contact_report = contact.contact_step(rc.arm_id, rc.N_JOINTS, params, q, dq, planes.astype(dtype),
                                                         None, report=True, dtype=dtype, device=rc.device)
        return tau

    def contact_report(self):
        """the report of the last send_forces: {"force", "force_local", "depth", "n_contacts"} (contact.report_dict), one
        row per arm; None before the first step or without surfaces"""
        return None if self._contact_report is None else contact.report_dict(self._contact_report)

    def _link_contact(self, q, dq, dtype):
        """-> the torque [B, n] of the state (q, dq) on self.obstacles; keeps the report"""
        rc, B = self.robot_config, q.shape[0]
        ob = self.obstacles
        if isinstance(ob, link_contact.Obstacles):
            spheres, params = link_contact.obstacle_rows(ob.obstacles, B), ob.params()
        else:
            spheres = link_contact.obstacle_rows(ob, B)
            params = _abi.make_link_contact_params(rc.N_JOINTS, n_obstacles=spheres.shape[1])
        tau, self._link_contact_report = link_contact.link_contact_step(
            rc.arm_id, rc.N_JOINTS, params, q, dq, spheres.astype(dtype), None, report=True, dtype=dtype,
            device=rc.device)
        return tau

    def link_contact_report(self):
        """the report of the last send_forces: {"force", "depth", "n_contacts", "segment", "obstacle", "t"}
        (link_contact.report_dict), one row per arm; None before the first step or without obstacles"""
        return None if self._link_contact_report is None else link_contact.report_dict(self._link_contact_report)

    def connect(self):
        self.reset()

    def disconnect(self):
        self.reset()

    def reset(self):
        self.q = np.copy(self.q_init)
        self.dq = np.zeros(self.q.shape)

    def get_feedback(self):
        return {"q": self.q, "dq": self.dq}

    def send_forces(self, u, dt=None, tau_ext=None, wrench=None):
        """advance one time step under torques u (arm_sim.py:67-82); tau_ext (n,) or (B, n) and wrench (6,) or (B, 6) are
        loads the controller does not know of; the payload carried is self.payload (set_payload changes it between steps);
        with surfaces and / or obstacles the contact is evaluated first and its torque added to tau_ext"""
        rc = self.robot_config
        dtype = np.dtype(getattr(rc, "dtype", np.float64))
        single = self.q.ndim == 1
        q = np.array(np.atleast_2d(self.q), dtype=dtype, order="C")
        dq = np.array(np.atleast_2d(self.dq), dtype=dtype, order="C")
        u2 = np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(u, dtype=dtype)), q.shape))
        params = _abi.make_plant_params(self.dt if dt is None else dt, self.substeps, self.gravity)

        def rows(x, w):
            if x is None:
                return None
            return np.ascontiguousarray(np.broadcast_to(np.atleast_2d(np.asarray(x, dtype=dtype)), (q.shape[0], w)))

        ext = rows(tau_ext, q.shape[1])
        if self.surfaces is not None:
            tau_c = self._contact(q, dq, dtype)
            ext = tau_c if ext is None else ext + tau_c
        if self.obstacles is not None:
            tau_l = self._link_contact(q, dq, dtype)
            ext = tau_l if ext is None else ext + tau_l
        plant_payload.plant_step(rc.arm_id, rc.N_JOINTS, params, q, dq, u2, dtype=dtype, device=rc.device,
                                 effects=self.effects, tau_ext=ext, wrench=rows(wrench, 6),
                                 payload=rows(self.payload, 4))
        self.q, self.dq = (q[0], dq[0]) if single else (q, dq)
        self.t += self.dt
