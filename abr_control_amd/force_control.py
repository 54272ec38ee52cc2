"""Force-controlled contact of a device-resident control loop: a hybrid motion/force law for the contact point.

One kernel (abrk_force_control_batch, include/abrk.h) is Khatib's unified motion/force law at p = Tx(frame, q, x=offset):
motion control (kp, kv) in the plane tangent to the surface normal n, a force PI loop (kf, ki, clamped at i_max) along n
while the sensed force n.F exceeds f_touch, a guarded approach along -n at v_app while it does not.  It is recordable into
an engine.Plan, reads a contact report as its force sensor, and reads its command at every launch:

    table = ContactSurfaces(rc, B, planes, stream=s)
    press = ForceController(rc, B, normal=(0, 0, 1), f_des=10.0, dt=1e-3, stream=s)
    rep = table.device_arrays()["report"].zero_(s)
    with engine.Plan(0, s) as tick:
        u = press.generate(q, dq, target, rep)                 # the force of the previous tick
        tau_c = table.apply(q, dq)
        engine.plant_step(rc.arm_id, n, plant, q, dq, u, stream=s, tau_ext=tau_c)
    tick.launch_graph(1500)
    press.set_command(f_des=15.0)                              # seen at the next replay
    tick.launch_graph(1000)

n is a unit vector of the world frame that points into free space; F is the force ON the tip.  Not modelled: orientation,
more than one constrained direction, Coriolis compensation, a moment about the point.
"""
import ctypes as C

import numpy as np

from . import _abi, engine
from ._lib import DeviceArray, check, lib
from .contact import REPORT_W

CMD_W = 4


def command_rows(normal, f_des, B):
    """normal [3] or [B,3], f_des a number or [B] -> a float64 array [B,4] = nx, ny, nz, f_des, checked as the C entry
    point checks a host array: finite, | |n| - 1 | <= 1e-6, f_des >= 0.  Raises ValueError naming the row."""
    B = int(B)
    nrm = np.asarray(normal, dtype=np.float64)
    if nrm.ndim == 1:
        nrm = np.broadcast_to(nrm, (B,) + nrm.shape)
    f = np.asarray(f_des, dtype=np.float64)
    if f.ndim == 0:
        f = np.broadcast_to(f, (B,))
    if nrm.shape != (B, 3) or f.shape != (B,):
        raise ValueError(f"normal has shape {np.shape(normal)} and f_des {np.shape(f_des)}; expected (3,) or ({B}, 3) "
                         f"and a number or ({B},)")
    cmd = np.ascontiguousarray(np.concatenate([nrm, f[:, None]], axis=1))
    finite = np.isfinite(cmd)
    if not finite.all():
        b, k = (int(x) for x in np.argwhere(~finite)[0])
        raise ValueError(f"cmd: row {b}: {_abi.FORCE_CMD[k]} is not finite")
    if (cmd[:, 3] < 0).any():
        b = int(np.argmax(cmd[:, 3] < 0))
        raise ValueError(f"cmd: row {b}: f_des={cmd[b, 3]:g} is negative")
    length = np.sqrt((cmd[:, :3] ** 2).sum(axis=1))
    if (np.abs(length - 1.0) > 1e-6).any():
        b = int(np.argmax(np.abs(length - 1.0) > 1e-6))
        raise ValueError(f"cmd: row {b}: |n|={length[b]:.9g} is not 1 to within 1e-6")
    return cmd


def force_control_step(arm_id, n, params, q, dq, target, cmd, force, integ, u=None, target_velocity=None,
                       dtype=np.float64, device=0, stream=None):
    """One tick of the law (abrk_force_control_batch) - recordable into a Plan.  params: _abi.make_force_params; q, dq
    [B,n]; target [B,6] (columns 0..2: x_d) and target_velocity [B,6] or None (columns 0..2: v_d); cmd [B,4] = nx, ny,
    nz, f_des; force [B, params.force_ld], columns 0..2 the force ON the tip in the world frame; integ [B], the force
    integral, updated in place; u [B,n] is written, or added to with params.accumulate (None: allocated here, not with
    accumulate).  All arrays of `dtype`, NumPy or DeviceArray alike.  A host cmd array is validated by the library, a
    DeviceArray is not.  -> u."""
    a = engine._Args(dtype, device)
    B = q.shape[0]
    qp, dqp = a.inp(q, (B, n), "q"), a.inp(dq, (B, n), "dq")
    tp, tvp = a.inp(target, (B, 6), "target"), a.inp(target_velocity, (B, 6), "target_velocity")
    cp = a.inp(cmd, (B, CMD_W), "cmd")
    fp = a.inp(force, (B, int(params.force_ld)), "force")
    ip = a.inout(integ, (B,), "integ")
    if ip is None:
        raise ValueError("integ, the force integral [B], is required")
    if params.accumulate:
        if u is None:
            raise ValueError("accumulate adds to u: pass the array")
        up, uo = a.inout(u, (B, n), "u"), u
    else:
        up, uo = a.out(u, (B, n), "u")
    check(lib().abrk_force_control_batch(arm_id, a.code, C.byref(params), B, qp, dqp, tp, tvp, cp, fp, ip, up, device,
                                         engine._sp(stream)))
    return uo


class ForceController:
    """The hybrid motion/force law for B rows of the arm `rc` (a robot_config of this package), with its command,
    integral and torque arrays on the device - as ContactSurfaces owns its arrays.

    normal: [3] (every row the same) or [B,3], unit, pointing into free space; f_des: a number or [B], >= 0 (N); gains:
    kp, kv, kf, ki, i_max, kvf, f_touch, v_app, kv_null and use_g as _abi.make_force_params takes them; frame / offset:
    the controlled point (as robot_config.Tx(frame, q, x=offset)); dt: the tick; dtype, device: the arm's unless given;
    stream: the stream generate(), set_command() and reset() run on."""

    def __init__(self, rc, B, normal, f_des, frame="EE", offset=(0, 0, 0), dt=0.001, dtype=None, device=None,
                 stream=None, **gains):
        B = int(B)
        if B < 1:
            raise ValueError(f"B={B} < 1")
        unknown = set(gains) - set(_abi.FORCE_GAINS) - {"use_g"}
        if unknown:
            raise TypeError(f"unknown gain(s) {sorted(unknown)}: one of {_abi.FORCE_GAINS + ('use_g',)}")
        self.rc, self.B, self.n, self.stream = rc, B, rc.N_JOINTS, stream
        self.dtype = engine._dtype_of(rc.dtype if dtype is None else dtype)[0]
        self.device = rc.device if device is None else device
        self.frame, self.offset, self.dt, self.gains = frame, tuple(float(x) for x in offset), float(dt), dict(gains)
        if isinstance(frame, str):
            rc.frame_id(frame)  # (an unknown name raises here, as robot_config.Tx does)
        self.params(3)  # (a malformed offset raises here)
        self.cmd = command_rows(normal, f_des, B)  # the host copy, float64 [B,4]
        self._cmd = DeviceArray.from_numpy(self.cmd.astype(self.dtype), self.device, engine._sp(stream))
        self._integ = DeviceArray((B,), self.dtype, self.device).zero_(stream)
        self._u = DeviceArray((B, self.n), self.dtype, self.device).zero_(stream)

    def params(self, force_ld, accumulate=False):
        """the _abi.ForceParams of this object's frame, offset, gains and dt for a force array of force_ld columns"""
        return _abi.make_force_params(self.n, self.frame, self.offset, dt=self.dt, accumulate=accumulate,
                                      force_ld=force_ld, **self.gains)

    def generate(self, q, dq, target, force, u=None, target_velocity=None, accumulate=False):
        """One tick (inside `with engine.Plan(...)`: recorded).  q, dq [B,n], target [B,6] and target_velocity [B,6] or
        None: DeviceArrays.  force: a DeviceArray [B,3] or wider whose columns 0..2 are the force ON the tip in the
        world frame - a ContactSurfaces report array ([B,8]) as it is.  u: the DeviceArray [B,n] to write, or with
        accumulate to add to (None: this object's own).  -> u."""
        if len(force.shape) != 2 or force.shape[0] != self.B or force.shape[1] < 3:
            raise ValueError(f"force has shape {tuple(force.shape)}; expected ({self.B}, 3) or wider "
                             f"(a contact report: ({self.B}, {REPORT_W}))")
        out = self._u if u is None else u
        return force_control_step(self.rc.arm_id, self.n, self.params(int(force.shape[1]), accumulate), q, dq, target,
                                  self._cmd, force, self._integ, u=out, target_velocity=target_velocity,
                                  dtype=self.dtype, device=self.device, stream=self.stream)

    def set_command(self, normal=None, f_des=None):
        """replace the normal ([3] or [B,3]) and / or the desired force (a number or [B]); what is None stays.  A copy
        on the object's stream, ordered with the ticks enqueued there before and after it - a recorded plan sees the
        new command at its next replay"""
        cmd = command_rows(self.cmd[:, :3] if normal is None else normal, self.cmd[:, 3] if f_des is None else f_des,
                           self.B)
        self.cmd = cmd
        self._cmd.copy_from_numpy(cmd.astype(self.dtype), self.stream)

    def reset(self):
        """zero the force integral (on the object's stream)"""
        self._integ.zero_(self.stream)

    def device_arrays(self):
        """{"cmd": [B,4], "integ": [B], "u": [B,n]}: the DeviceArrays themselves"""
        return {"cmd": self._cmd, "integ": self._integ, "u": self._u}
