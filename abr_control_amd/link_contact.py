"""Whole-arm contact of a device-resident control loop: the link segments as capsules against per-row sphere obstacles.

One kernel (abrk_link_contact_step_batch, include/abrk.h) finds the closest point of every link segment - joint_i to
joint_i+1, the last one to the EE: the segments of AvoidObstacles - to each of the row's own spheres and turns
penetration into the joint torque tau_c = sum Jx^T f - Kelvin-Voigt normal force without adhesion, smoothed Coulomb
friction, the law of contact.py - where the plant reads its joint-space disturbance.  It is recordable into an
engine.Plan, and the kernel reads the obstacles at every launch:

    world = Obstacles.from_controller(avoid, B, k=2e4, c=40.0, stream=s)     # the spheres the loop avoids
    with engine.Plan(0, s) as tick:
        engine.osc_generate(rc.arm_id, n, law, q, dq, target, u=u, stream=s)
        tau_c = world.apply(q, dq)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=s, tau_ext=tau_c)
    tick.launch_graph(1000)
    world.report()["depth"]        # [B]: negative - the arm stayed clear

The force is evaluated once per tick, from the state at the start of the tick, and the plant holds it over its substeps
like u: include/abrk.h states the stability bound on k dt^2 / m_eff this implies.
"""
import ctypes as C

import numpy as np

from . import _abi, engine
from ._lib import DeviceArray, check, lib

REPORT_W = 8


def obstacle_rows(obstacles, B):
    """obstacles [K,7] (every row the same) or [B,K,7] -> a float64 array [B,K,7], checked as the C entry point checks
    a host array: finite, R > 0, k, c, mu >= 0, 1 <= K <= 8.  Raises ValueError naming row, obstacle and column."""
    p = np.asarray(obstacles, dtype=np.float64)
    if p.ndim == 2:
        p = np.broadcast_to(p, (int(B),) + p.shape)
    if p.ndim != 3 or p.shape[0] != int(B) or p.shape[2] != 7 or not 1 <= p.shape[1] <= _abi.LINK_CONTACT_MAX_OBSTACLES:
        raise ValueError(f"obstacles has shape {np.shape(obstacles)}; expected (K, 7) or ({int(B)}, K, 7) with K in "
                         f"1..{_abi.LINK_CONTACT_MAX_OBSTACLES}")
    p = np.ascontiguousarray(p)

    def first(mask):
        return tuple(int(x) for x in np.argwhere(mask)[0])

    finite = np.isfinite(p)
    if not finite.all():
        b, o, k = first(~finite)
        raise ValueError(f"obstacles: row {b}, obstacle {o}: {_abi.LINK_OBSTACLE[k]} is not finite")
    if (p[:, :, 3] <= 0).any():
        b, o = first(p[:, :, 3] <= 0)
        raise ValueError(f"obstacles: row {b}, obstacle {o}: R={p[b, o, 3]:g} is not > 0")
    if (p[:, :, 4:] < 0).any():
        b, o, k = first(p[:, :, 4:] < 0)
        raise ValueError(f"obstacles: row {b}, obstacle {o}: {_abi.LINK_OBSTACLE[4 + k]}={p[b, o, 4 + k]:g} is negative")
    return p


def link_contact_step(arm_id, n, params, q, dq, obstacle, tau, report=None, dtype=np.float64, device=0, stream=None):
    """One tick of the whole-arm contact (abrk_link_contact_step_batch) - recordable into a Plan.  params:
    _abi.make_link_contact_params; q, dq [B,n]; obstacle [B,K,7] = cx, cy, cz, R, k, c, mu with K = params.n_obstacles;
    tau [B,n] is written, or added to with params.accumulate (None: allocated here, not with accumulate); report: None,
    True or a [B,8] array - F in the world frame, the deepest penetration, the pairs penetrated, then segment, obstacle
    and t of the deepest pair.  All arrays of `dtype`, NumPy or DeviceArray alike.  A host obstacle array is validated
    by the library, a DeviceArray is not.  -> tau, or (tau, report)."""
    a = engine._Args(dtype, device)
    B = q.shape[0]
    K = int(params.n_obstacles)
    qp, dqp = a.inp(q, (B, n), "q"), a.inp(dq, (B, n), "dq")
    op = a.inp(obstacle, (B, K, 7), "obstacle")
    if params.accumulate:
        if tau is None:
            raise ValueError("accumulate adds to tau: pass the array")
        tp, to = a.inout(tau, (B, n), "tau"), tau
    else:
        tp, to = a.out(tau, (B, n), "tau")
    rp, ro = a.opt_out(report, (B, REPORT_W), "report")
    check(lib().abrk_link_contact_step_batch(arm_id, a.code, C.byref(params), B, qp, dqp, op, tp, rp, device,
                                             engine._sp(stream)))
    return to if ro is None else (to, ro)


def report_dict(report):
    """report [B,8] -> {"force": [B,3] world frame, "depth": [B] the deepest penetration (negative: clear of
    everything), "n_contacts": [B] pairs penetrated, "segment", "obstacle": [B] of the deepest pair, "t": [B] where on
    that segment (0: at joint_i, 1: at its far end)}"""
    r = np.asarray(report)
    return {"force": r[:, 0:3].copy(), "depth": r[:, 3].copy(), "n_contacts": r[:, 4].astype(np.int64),
            "segment": r[:, 5].astype(np.int64), "obstacle": r[:, 6].astype(np.int64), "t": r[:, 7].copy()}


class Obstacles:
    """The sphere obstacles of B rows of the arm `rc` (a robot_config of this package), with the torque and report
    arrays of the link-contact step, all on the device - the shape of contact.ContactSurfaces.

    obstacles: [K,7] (every row the same) or [B,K,7] of cx, cy, cz, R, k, c, mu - centre and radius (m), stiffness k
    (N/m), damping c (N s/m), friction coefficient mu; link_radius: the radius of the segment capsules, a scalar or N
    values (< 0: that segment is off); vs: the smoothing speed of the friction law; dtype, device: the arm's unless
    given; stream: the stream apply(), set_obstacles() and report() run on."""

    def __init__(self, rc, B, obstacles, link_radius=0.04, vs=1e-3, dtype=None, device=None, stream=None):
        B = int(B)
        if B < 1:
            raise ValueError(f"B={B} < 1")
        self.rc, self.B, self.n, self.stream = rc, B, rc.N_JOINTS, stream
        self.dtype = engine._dtype_of(rc.dtype if dtype is None else dtype)[0]
        self.device = rc.device if device is None else device
        self.vs = float(vs)
        if not (np.isfinite(self.vs) and self.vs > 0):
            raise ValueError(f"vs={vs} is not a finite value > 0")
        r = np.asarray(link_radius, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(self.n, float(r))
        if r.shape != (self.n,) or not np.isfinite(r).all() or not (r >= 0).any():
            raise ValueError(f"link_radius={link_radius}: expected a finite scalar or {self.n} finite values, not all < 0")
        self.link_radius = r
        self.obstacles = obstacle_rows(obstacles, B)  # the host copy, float64 [B,K,7]
        self.K = self.obstacles.shape[1]
        self._obstacle = DeviceArray.from_numpy(self.obstacles.astype(self.dtype), self.device, engine._sp(stream))
        self._tau = DeviceArray((B, self.n), self.dtype, self.device).zero_(stream)
        self._report = DeviceArray((B, REPORT_W), self.dtype, self.device).zero_(stream)

    @classmethod
    def from_controller(cls, avoid, B, k, c, mu=0.0, **kw):
        """the spheres an AvoidObstacles controller avoids ([[x, y, z, r], ...], the same for every row) as the spheres
        the arm can hit, all with stiffness k, damping c and friction mu"""
        xyzr = np.asarray(avoid.obstacles, dtype=np.float64).reshape(-1, 4)
        rows = np.concatenate([xyzr, np.tile([float(k), float(c), float(mu)], (xyzr.shape[0], 1))], axis=1)
        return cls(avoid.robot_config, B, rows, **kw)

    def params(self, accumulate=False):
        """the _abi.LinkContactParams of this object's obstacle count, radii and vs"""
        return _abi.make_link_contact_params(self.n, self.K, self.link_radius, self.vs, accumulate)

    def apply(self, q, dq, tau=None, accumulate=False):
        """One tick (inside `with engine.Plan(...)`: recorded).  q, dq: DeviceArrays [B,n].  tau: the DeviceArray [B,n]
        to write, or with accumulate to add to (None: this object's own).  -> tau: pass it as tau_ext= to
        engine.plant_step or plant_payload.plant_step.  The report is refreshed by every call."""
        out = self._tau if tau is None else tau
        link_contact_step(self.rc.arm_id, self.n, self.params(accumulate), q, dq, self._obstacle, out,
                          report=self._report, dtype=self.dtype, device=self.device, stream=self.stream)
        return out

    def set_obstacles(self, obstacles):
        """replace the obstacles, [K,7] or [B,K,7] with the K this object was made with: a copy on the object's stream,
        ordered with the ticks enqueued there before and after it - a recorded plan sees them at its next replay"""
        p = obstacle_rows(obstacles, self.B)
        if p.shape[1] != self.K:
            raise ValueError(f"this object holds {self.K} obstacles per row; got {p.shape[1]}")
        self.obstacles = p
        self._obstacle.copy_from_numpy(p.astype(self.dtype), self.stream)

    def report(self):
        """the report of the last tick as NumPy arrays: {"force", "depth", "n_contacts", "segment", "obstacle", "t"}"""
        return report_dict(self._report.numpy(self.stream))

    def device_arrays(self):
        """{"obstacle": [B,K,7], "tau": [B,n], "report": [B,8]}: the DeviceArrays themselves"""
        return {"obstacle": self._obstacle, "tau": self._tau, "report": self._report}
