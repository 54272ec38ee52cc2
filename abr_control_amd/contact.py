"""End-effector contact of a device-resident control loop: per-row planes, a sphere tip, a force report.

One kernel (abrk_contact_step_batch, include/abrk.h) turns the penetration of the tip at p = Tx(frame, q, x=offset) into
each row's own half-spaces into the joint torque tau_c = Jp^T F - Kelvin-Voigt normal force without adhesion, smoothed
Coulomb friction - and writes it where the plant reads its joint-space disturbance.  It is recordable into an
engine.Plan, and the kernel reads the planes at every launch:

    table = ContactSurfaces(rc, B, planes, stream=s)          # planes [S,8] or [B,S,8]: nx, ny, nz, d, k, c, mu, rho
    with engine.Plan(0, s) as tick:
        engine.osc_generate(rc.arm_id, n, law, q, dq, target, u=u, stream=s)
        tau_c = table.apply(q, dq)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=s, tau_ext=tau_c)
    tick.launch_graph(1000)
    table.report()["force"]        # [B,3], world frame

The force is evaluated once per tick, from the state at the start of the tick, and the plant holds it over its substeps
like u: include/abrk.h states the stability bound on k dt^2 / m_eff this implies.
"""
import ctypes as C

import numpy as np

from . import _abi, engine
from ._lib import DeviceArray, check, lib

REPORT_W = 8


def planes_rows(planes, B):
    """planes [S,8] (every row the same) or [B,S,8] -> a float64 array [B,S,8], checked as the C entry point checks a
    host array: finite, | |n| - 1 | <= 1e-6, k, c, mu, rho >= 0, 1 <= S <= 4.  Raises ValueError naming row and surface."""
    p = np.asarray(planes, dtype=np.float64)
    if p.ndim == 2:
        p = np.broadcast_to(p, (int(B),) + p.shape)
    if p.ndim != 3 or p.shape[0] != int(B) or p.shape[2] != 8 or not 1 <= p.shape[1] <= _abi.CONTACT_MAX_SURFACES:
        raise ValueError(f"planes has shape {np.shape(planes)}; expected (S, 8) or ({int(B)}, S, 8) with S in "
                         f"1..{_abi.CONTACT_MAX_SURFACES}")
    p = np.ascontiguousarray(p)

    def first(mask):
        return tuple(int(x) for x in np.argwhere(mask)[0])

    finite = np.isfinite(p)
    if not finite.all():
        b, s, k = first(~finite)
        raise ValueError(f"planes: row {b}, surface {s}: {_abi.CONTACT_SURFACE[k]} is not finite")
    if (p[:, :, 4:] < 0).any():
        b, s, k = first(p[:, :, 4:] < 0)
        raise ValueError(f"planes: row {b}, surface {s}: {_abi.CONTACT_SURFACE[4 + k]}={p[b, s, 4 + k]:g} is negative")
    length = np.sqrt((p[:, :, :3] ** 2).sum(axis=2))
    if (np.abs(length - 1.0) > 1e-6).any():
        b, s = first(np.abs(length - 1.0) > 1e-6)
        raise ValueError(f"planes: row {b}, surface {s}: |n|={length[b, s]:.9g} is not 1 to within 1e-6")
    return p


def contact_step(arm_id, n, params, q, dq, surface, tau, report=None, dtype=np.float64, device=0, stream=None):
    """One tick of the contact (abrk_contact_step_batch) - recordable into a Plan.  params: _abi.make_contact_params; q,
    dq [B,n]; surface [B,S,8] = nx, ny, nz, d, k, c, mu, rho with S = params.n_surfaces; tau [B,n] is written, or added
    to with params.accumulate (None: allocated here, not with accumulate); report: None, True or a [B,8] array - F in
    the world frame, F in the frame's coordinates, the deepest penetration, the number of surfaces penetrated.  All
    arrays of `dtype`, NumPy or DeviceArray alike.  A host surface array is validated by the library, a DeviceArray is
    not.  -> tau, or (tau, report)."""
    a = engine._Args(dtype, device)
    B = q.shape[0]
    S = int(params.n_surfaces)
    qp, dqp = a.inp(q, (B, n), "q"), a.inp(dq, (B, n), "dq")
    sp = a.inp(surface, (B, S, 8), "surface")
    if params.accumulate:
        if tau is None:
            raise ValueError("accumulate adds to tau: pass the array")
        tp, to = a.inout(tau, (B, n), "tau"), tau
    else:
        tp, to = a.out(tau, (B, n), "tau")
    rp, ro = a.opt_out(report, (B, REPORT_W), "report")
    check(lib().abrk_contact_step_batch(arm_id, a.code, C.byref(params), B, qp, dqp, sp, tp, rp, device,
                                        engine._sp(stream)))
    return to if ro is None else (to, ro)


def report_dict(report):
    """report [B,8] -> {"force": [B,3] world frame, "force_local": [B,3] in the frame's coordinates, "depth": [B] the
    deepest penetration (negative: clear of every surface), "n_contacts": [B] surfaces penetrated}"""
    r = np.asarray(report)
    return {"force": r[:, 0:3].copy(), "force_local": r[:, 3:6].copy(), "depth": r[:, 6].copy(),
            "n_contacts": r[:, 7].astype(np.int64)}


class ContactSurfaces:
    """The planes of B rows of the arm `rc` (a robot_config of this package), with the torque and report arrays of the
    contact step, all on the device - as JointSensor owns its arrays.

    planes: [S,8] (every row the same) or [B,S,8] of nx, ny, nz, d, k, c, mu, rho - unit normal n, free side n.x > d,
    stiffness k (N/m), damping c (N s/m), friction coefficient mu, tip radius rho (m); frame / offset: the contact point
    (as robot_config.Tx(frame, q, x=offset)); vs: the smoothing speed of the friction law; dtype, device: the arm's
    unless given; stream: the stream apply(), set_planes() and report() run on."""

    def __init__(self, rc, B, planes, frame="EE", offset=(0, 0, 0), vs=1e-3, dtype=None, device=None, stream=None):
        B = int(B)
        if B < 1:
            raise ValueError(f"B={B} < 1")
        self.rc, self.B, self.n, self.stream = rc, B, rc.N_JOINTS, stream
        self.dtype = engine._dtype_of(rc.dtype if dtype is None else dtype)[0]
        self.device = rc.device if device is None else device
        self.frame, self.offset, self.vs = frame, tuple(float(x) for x in offset), float(vs)
        if not (np.isfinite(self.vs) and self.vs > 0):
            raise ValueError(f"vs={vs} is not a finite value > 0")
        self.planes = planes_rows(planes, B)  # the host copy, float64 [B,S,8]
        self.S = self.planes.shape[1]
        if isinstance(frame, str):
            rc.frame_id(frame)  # (an unknown name raises here, as robot_config.Tx does)
        self._surface = DeviceArray.from_numpy(self.planes.astype(self.dtype), self.device, engine._sp(stream))
        self._tau = DeviceArray((B, self.n), self.dtype, self.device).zero_(stream)
        self._report = DeviceArray((B, REPORT_W), self.dtype, self.device).zero_(stream)

    def params(self, accumulate=False):
        """the _abi.ContactParams of this object's frame, offset, surface count and vs"""
        return _abi.make_contact_params(self.n, self.frame, self.offset, self.S, self.vs, accumulate)

    def apply(self, q, dq, tau=None, accumulate=False):
        """One tick (inside `with engine.Plan(...)`: recorded).  q, dq: DeviceArrays [B,n].  tau: the DeviceArray [B,n]
        to write, or with accumulate to add to (None: this object's own).  -> tau: pass it as tau_ext= to
        engine.plant_step or plant_payload.plant_step.  The report is refreshed by every call."""
        out = self._tau if tau is None else tau
        contact_step(self.rc.arm_id, self.n, self.params(accumulate), q, dq, self._surface, out, report=self._report,
                     dtype=self.dtype, device=self.device, stream=self.stream)
        return out

    def set_planes(self, planes):
        """replace the planes, [S,8] or [B,S,8] with the S this object was made with: a copy on the object's stream,
        ordered with the ticks enqueued there before and after it - a recorded plan sees the new planes at its next replay"""
        p = planes_rows(planes, self.B)
        if p.shape[1] != self.S:
            raise ValueError(f"this object holds {self.S} surfaces per row; got {p.shape[1]}")
        self.planes = p
        self._surface.copy_from_numpy(p.astype(self.dtype), self.stream)

    def report(self):
        """the report of the last tick as NumPy arrays: {"force", "force_local", "depth", "n_contacts"} (report_dict)"""
        return report_dict(self._report.numpy(self.stream))

    def device_arrays(self):
        """{"surface": [B,S,8], "tau": [B,n], "report": [B,8]}: the DeviceArrays themselves"""
        return {"surface": self._surface, "tau": self._tau, "report": self._report}
